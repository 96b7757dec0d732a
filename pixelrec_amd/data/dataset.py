"""Train / eval batch construction for the SASRec family (reference REC/data/dataset/{trainset,evalset,
collate_fn}.py) plus a vectorised whole-batch builder.

Reference semantics kept:
  * SEQTrainDataset item = (items [2, L+1], masked_index [L]): positives left-padded with 0; ONE negative per
    target position, uniform over [1, N-1] rejecting the sequence's own items (trainset.py:40-44), right-aligned
    (neg[0] is always 0); masked_index = 1 on the len-1 target positions (trainset.py:46-75);
  * SeqEvalDataset item = (history tensor, last-L left-padded item_seq, target): valid = [:-2] / [-2],
    test = [:-1] / [-1] (evalset.py:17-34); seq_eval_collate stacks them and emits the (history_u, history_i)
    pairs used to mask the whole history at eval (collate_fn.py:6-32).
What is new: the batchers build whole batches with numpy (the per-sample Python `random` loop in 10 worker
processes is the bottleneck once a step takes ~2 ms on the GPU).  Every train batcher is a
`TrainBatcher` (the order, the epoch's rng, iteration) with its own make_batch; every eval batcher is a `SeqEvalBatcher`
with its own model_input.  tests/test_batcher_streams_cpu.py pins what each of them yields.
"""
from __future__ import annotations

import functools
import random

import numpy as np
import torch
from torch.utils.data import Dataset


class SEQTrainDataset(Dataset):
    def __init__(self, config, dataload):
        self.dataload = dataload
        self.item_num = dataload.item_num
        self.train_seq = dataload.train_feat["item_seq"]
        self.length = len(self.train_seq)
        self.max_seq_length = config["MAX_ITEM_LIST_LENGTH"] + 1

    def __len__(self):
        return self.length

    def _neg_sample(self, item_set):
        item = random.randint(1, self.item_num - 1)
        while item in item_set:
            item = random.randint(1, self.item_num - 1)
        return item

    @staticmethod
    def _pad(sequence, max_length):
        sequence = [0] * (max_length - len(sequence)) + list(sequence)
        return torch.tensor(sequence[-max_length:], dtype=torch.long)

    def __getitem__(self, index):
        item_seq = self.train_seq[index]
        n = len(item_seq)
        neg = [self._neg_sample(item_seq) for _ in range(n - 1)]
        mask = [1] * (n - 1)
        return (torch.stack((self._pad(list(item_seq), self.max_seq_length), self._pad(neg, self.max_seq_length))),
                self._pad(mask, self.max_seq_length - 1))


class BERT4RecTrainDataset(Dataset):
    """Reference BERT4RecTrainDataset (REC/data/dataset/trainset.py:418-479), per sample: each real position of the window is
    masked with probability mask_ratio -- the mask token item_num in the masked sequence, a negative outside the sequence, 1 in
    masked_index -- and the planes are left-padded AFTER masking, so padding is never masked.
    item = (items [3, L+1] = masked sequence | original sequence | negatives, masked_index [L+1])."""

    def __init__(self, config, dataload):
        self.dataload = dataload
        self.item_num = dataload.item_num
        self.train_seq = dataload.train_feat["item_seq"]
        self.length = len(self.train_seq)
        self.max_seq_length = config["MAX_ITEM_LIST_LENGTH"] + 1
        self.mask_ratio = config["mask_ratio"]
        self.mask_token = self.item_num

    def __len__(self):
        return self.length

    def _neg_sample(self, item_set):
        item = random.randint(1, self.item_num - 1)
        while item in item_set:
            item = random.randint(1, self.item_num - 1)
        return item

    def __getitem__(self, index):
        item_seq = list(self.train_seq[index])
        neg, masked, mask = [], [], []
        for item in item_seq:
            if random.random() < self.mask_ratio:
                neg.append(self._neg_sample(item_seq))
                masked.append(self.mask_token)
                mask.append(1)
            else:
                neg.append(0)
                masked.append(item)
                mask.append(0)
        pad = lambda x: SEQTrainDataset._pad(x, self.max_seq_length)
        return torch.stack((pad(masked), pad(item_seq), pad(neg))), pad(mask)


class SeqEvalDataset(Dataset):
    def __init__(self, config, dataload, phase="valid"):
        self.dataload = dataload
        self.max_item_list_length = config["MAX_ITEM_LIST_LENGTH"]
        self.user_seq = list(dataload.user_seq.values())
        self.phase = phase
        self.length = len(self.user_seq)
        self.item_num = dataload.item_num

    def __len__(self):
        return self.length

    def _padding_sequence(self, sequence, max_length):
        sequence = [0] * (max_length - len(sequence)) + list(sequence)
        return sequence[-max_length:]

    def __getitem__(self, index):
        seq = self.user_seq[index]
        if self.phase == "valid":
            history_seq, item_target = seq[:-2], seq[-2]
        else:
            history_seq, item_target = seq[:-1], seq[-1]
        item_seq = self._padding_sequence(history_seq, self.max_item_list_length)
        return torch.tensor(np.asarray(history_seq, dtype=np.int64)), item_seq, int(item_target)


def seq_eval_collate(batch):
    history_i = [item[0] for item in batch]
    item_seq = torch.tensor([item[1] for item in batch], dtype=torch.long)
    item_target = torch.tensor([item[2] for item in batch], dtype=torch.long)
    history_u = torch.cat([torch.full_like(h, i) for i, h in enumerate(history_i)])
    history_i = torch.cat(history_i)
    positive_u = torch.arange(item_seq.shape[0])
    return item_seq, (history_u, history_i), positive_u, item_target


# ---- what the batchers share -------------------------------------------------------------------------------------------

def left_padded_windows(seqs, W):
    """A list of sequences of at most W items -> (windows int64 [n, W], left-padded with 0; lens int64 [n])."""
    windows = np.zeros((len(seqs), W), dtype=np.int64)
    lens = np.zeros(len(seqs), dtype=np.int64)
    for i, s in enumerate(seqs):
        k = len(s)
        windows[i, W - k:] = s
        lens[i] = k
    return windows, lens


def gather_windows(flat, start, count, W, left_pad):
    """CSR rows flat[start[b] : start[b] + count[b]] -> int64 [B, W], padded with 0.  left_pad: the row's LAST min(count, W) items,
    right-aligned; otherwise its FIRST min(count, W) items, left-aligned.  count <= 0 gives an empty row."""
    col = np.arange(W, dtype=np.int64)[None, :]
    if left_pad:
        src = (count - W)[:, None] + col                               # position inside the row
        ok = src >= 0
    else:
        src, ok = col, col < count[:, None]
    return np.where(ok, flat[np.where(ok, start[:, None] + src, 0)], 0)


def redraw_clashes(neg, clashes, rng, item_num, bound, who):
    """Rejection sampling after the caller's first draw `neg` (uniform over [1, item_num - 1], any shape): while clashes(neg) -> bool
    array marks any entry, those entries are redrawn in place, one rng.integers call per round.  At most `bound` rounds, None for
    no limit.  After the last round `who` = None returns neg as it stands (clashes and all); otherwise ValueError names `who`."""
    tries = 0
    while bound is None or tries < bound:
        clash = clashes(neg)
        if not clash.any():
            return neg
        neg[clash] = rng.integers(1, item_num, size=int(clash.sum()))
        tries += 1
    if who is not None:
        raise ValueError(f"{who} covers (nearly) every item: no negative could be drawn")
    return neg


def _in_row(win):
    """clashes() of one negative per row of `win` [B, W].  Negatives are >= 1, so the 0 padding of a row never clashes."""
    return lambda neg: (neg[:, None] == win).any(1)


def _in_row_at(win, where):
    """clashes() of one negative per position of `win` [B, W], looked at on the positions `where` [B, W] only."""
    return lambda neg: (neg[:, :, None] == win[:, None, :]).any(-1) & where


class TrainBatcher:
    """The frame of every train batcher: whole batches, built with numpy, in the order of DataLoader(sampler=DistributedSampler).
      * order: _indices() reproduces torch's DistributedSampler (shuffle with generator seed = seed + epoch, pad to a multiple of
        world by wrapping, rank-strided) over `n` units; batch b is rows = _indices()[b * batch_size : (b + 1) * batch_size];
      * randomness: one numpy Generator per epoch, keyed [config seed, epoch, rank], handed to every make_batch of the epoch in
        batch order -- the stream is a function of (seed, epoch, rank) alone, so a resumed run redraws what the first run drew;
      * make_batch(rows, rng) -> tuple of numpy arrays: a pure function of (rows, the rng's state); it draws from `rng` only, in
        a fixed order, and keeps no state between calls.  Iteration yields the same tuple as torch tensors (no copy).
    A subclass prepares its arrays in __init__, names its unit count with _set_units(n) and defines make_batch."""

    def __init__(self, config, dataload, rank=0, world=1, seed=0, drop_last=False):
        self.dataload = dataload
        self.item_num = dataload.item_num
        self.batch_size = config["train_batch_size"]
        self.rank, self.world, self.seed, self.epoch = rank, world, seed, 0
        self.drop_last = drop_last
        self.neg_seed = int(config["seed"] or 0)

    def _set_units(self, n):
        """n = the number of units the order runs over (samples; MoPoolTrainBatcher: chunks)."""
        self.n = n
        self.num_samples = -(-n // self.world)

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return self.num_samples // self.batch_size if self.drop_last else -(-self.num_samples // self.batch_size)

    def _indices(self):
        g = torch.Generator()
        g.manual_seed(self.seed + self.epoch)
        idx = torch.randperm(self.n, generator=g).tolist()
        total = self.num_samples * self.world
        pad = total - len(idx)
        if pad > 0:
            idx += (idx * ((pad + len(idx) - 1) // len(idx) + 1))[:pad]
        return np.asarray(idx[self.rank:total:self.world], dtype=np.int64)

    def _batch_rows(self):
        idx = self._indices()
        for b in range(len(self)):
            yield idx[b * self.batch_size:(b + 1) * self.batch_size]

    def make_batch(self, rows, rng):
        raise NotImplementedError

    def __iter__(self):
        rng = np.random.default_rng([self.neg_seed, self.epoch, self.rank])
        for rows in self._batch_rows():
            yield tuple(torch.from_numpy(x) for x in self.make_batch(rows, rng))


class SeqTrainBatcher(TrainBatcher):
    """Vectorised equivalent of DataLoader(SEQTrainDataset, sampler=DistributedSampler): yields whole
    (items [B,2,L+1], masked_index [B,L]) int64 batches."""

    def __init__(self, config, dataload, rank=0, world=1, seed=0, drop_last=False):
        super().__init__(config, dataload, rank=rank, world=world, seed=seed, drop_last=drop_last)
        self.W = config["MAX_ITEM_LIST_LENGTH"] + 1
        self.windows, self.lens = left_padded_windows(dataload.train_feat["item_seq"], self.W)
        self._set_units(len(self.windows))
        # device_sampler: yield only the positive windows ([B, L+1] int64, pinned-copy friendly); the negatives and
        # the mask are then drawn on the GPU by ops.sample_negatives (pxr_sample_negatives_i64) -- the host work per
        # batch drops from ~0.8 ms of numpy to one fancy-index gather
        try:
            ds = config["device_sampler"]       # Config returns None for missing keys, plain dicts raise
        except KeyError:
            ds = None
        self.device_sampler = bool(ds) if ds is not None else False

    def make_batch(self, rows, rng):
        pos = self.windows[rows]                                   # [B, W]
        lens = self.lens[rows]
        B, W = pos.shape
        col = np.arange(W)[None, :]
        tgt = col >= (W - lens[:, None] + 1)                       # target positions: the last len-1 columns
        neg = rng.integers(1, self.item_num, size=(B, W))
        if self.item_num > 2 * W:                                  # rejection of the sequence's own items: 64 rounds, then as is
            redraw_clashes(neg, _in_row_at(pos, tgt), rng, self.item_num, bound=64, who=None)
        neg = np.where(tgt, neg, 0)
        items = np.stack((pos, neg), axis=1)
        return items, tgt[:, 1:].astype(np.int64)

    def estimate_exchange_rows(self, n_batches: int = 64, margin: float = 1.25) -> int:
        """A row capacity for the data-parallel exchange of the sparse table gradient (`dp_exchange_rows: auto`): the
        largest number of distinct item ids among the first `n_batches` batches of this rank's epoch-0 order (negatives
        drawn like the host sampler does), times `margin`, rounded up to 256 and capped at the worst case B*(2L+1).  It is
        a statistical bound -- a later batch that exceeds it sets the status word and the trainer raises at its next host
        sync (pxr_merge_split_rows_f32) -- and it costs no training state: the batcher's random streams are functions of
        (seed, epoch, rank) only."""
        worst = self.batch_size * (2 * self.W - 1)
        idx = self._indices()
        rng = np.random.default_rng([self.neg_seed, 0, self.rank, 12345])
        top = 0
        for b in range(min(n_batches, len(self))):
            rows = idx[b * self.batch_size:(b + 1) * self.batch_size]
            items, _ = self.make_batch(rows, rng)
            top = max(top, int(np.count_nonzero(np.unique(items))))
        return int(min(worst, (int(top * margin) + 255) // 256 * 256))

    def _device_sampler_batches(self):
        # (windows, batch id): the consumer turns them into (items, mask) on the device
        for b, rows in enumerate(self._batch_rows()):
            yield torch.from_numpy(self.windows[rows]), (self.neg_seed, (self.epoch << 32) | (self.rank << 24) | b)

    def __iter__(self):
        return self._device_sampler_batches() if self.device_sampler else super().__iter__()


class BERT4RecTrainBatcher(SeqTrainBatcher):
    """Vectorised BERT4RecTrainDataset over SeqTrainBatcher's windows and sample order: yields whole (items [B,3,L+1],
    masked_index [B,L+1]) int64 batches.  Same distribution as the reference (Bernoulli(mask_ratio) per real position, negatives
    uniform over [1, item_num-1] rejecting the sequence's own items), not the same random stream."""

    def __init__(self, config, dataload, rank=0, world=1, seed=0, drop_last=False):
        super().__init__(config, dataload, rank=rank, world=world, seed=seed, drop_last=drop_last)
        self.mask_ratio = float(config["mask_ratio"])
        self.mask_token = self.item_num
        self.device_sampler = False      # the device-side sampler draws SASRec's batches only

    def make_batch(self, rows, rng):
        pos = self.windows[rows]                                   # [B, W], left-padded
        lens = self.lens[rows]
        B, W = pos.shape
        real = np.arange(W)[None, :] >= (W - lens[:, None])        # the sequence's own positions (never the padding)
        masked = real & (rng.random((B, W)) < self.mask_ratio)
        neg = rng.integers(1, self.item_num, size=(B, W))
        # rejection of the sequence's own items: 64 rounds, then as is
        redraw_clashes(neg, _in_row_at(pos, masked), rng, self.item_num, bound=64, who=None)
        neg = np.where(masked, neg, 0)
        inp = np.where(masked, self.mask_token, pos)
        items = np.stack((inp, pos, neg), axis=1)
        return items, masked.astype(np.int64)


class TwoTowerTrainBatcher(TrainBatcher):
    """Vectorised TwoTowerTrainDataset (reference REC/data/dataset/trainset.py:256-290).  The reference tags LightSANs AUGSEQ, so its
    train_feat['item_seq'] holds every prefix of length >= 2 of every training chunk (Data._build_aug_seq, as for SRGNN) and each
    prefix is one row: the prefix followed by one negative, left-padded with 0 to L+2.  The negative is uniform over
    [1, item_num - 1] and redrawn while it lies in the prefix, target included -- the reference's distribution, not its random
    stream.  Yields whole (history int64 [B, L] = row[:, :L], target int64 [B, 2] = (row[:, L], row[:, L+1])) batches: the two
    tensors the training loop stages (LightSANs.forward joins them)."""

    def __init__(self, config, dataload, rank=0, world=1, seed=0, drop_last=False):
        super().__init__(config, dataload, rank=rank, world=world, seed=seed, drop_last=drop_last)
        self.L = config["MAX_ITEM_LIST_LENGTH"]
        if "seq_start" not in dataload.train_feat:
            raise ValueError("TwoTowerTrainBatcher reads the AUGSEQ prefixes: build the data with MODEL_INPUT_TYPE = AUGSEQ")
        self.flat = np.asarray(dataload._sorted_items, dtype=np.int64)
        self.start = np.asarray(dataload.train_feat["seq_start"], dtype=np.int64)
        self.length = np.asarray(dataload.train_feat["seq_len"], dtype=np.int64)
        self._set_units(len(self.start))
        if self.item_num <= 2:
            raise ValueError("TwoTowerTrainBatcher: no negative can be drawn from [1, item_num) outside a prefix")

    def make_batch(self, rows, rng):
        W = self.L + 1
        win = gather_windows(self.flat, self.start[rows], self.length[rows], W, left_pad=True)   # prefix length: 2 .. L+1
        neg = rng.integers(1, self.item_num, size=len(win))
        redraw_clashes(neg, _in_row(win), rng, self.item_num, bound=1000, who="TwoTowerTrainBatcher: a prefix")
        return win[:, :W - 1].copy(), np.stack((win[:, W - 1], neg), axis=1)


class SampleAcfTrainBatcher(TrainBatcher):
    """Vectorised SampleACFTrainDataset (reference REC/data/dataset/trainset.py:603-652).  Data builds the SEQ chunks of at most L+1
    items with their user id; every position j of every chunk is one sample: profile = the chunk without item j (order kept,
    left-padded with 0 to L), positive = item j, one negative uniform over [1, item_num - 1] and redrawn while it lies in the
    chunk -- the reference's distribution, not its random stream.  A chunk of one item gives one sample with an empty profile.
    The number of samples is the sum of the chunk lengths.  Yields whole (profile int64 [B, L], tail int64 [B, 3] = (positive,
    negative, user id)) batches: the two tensors the training loop stages (ACF.forward joins them into the reference's
    [B, L + 3] row)."""

    def __init__(self, config, dataload, rank=0, world=1, seed=0, drop_last=False):
        super().__init__(config, dataload, rank=rank, world=world, seed=seed, drop_last=drop_last)
        self.L = config["MAX_ITEM_LIST_LENGTH"]
        W = self.L + 1
        self.windows, self.lens = left_padded_windows(dataload.train_feat["item_seq"], W)     # the chunks
        lens = self.lens
        self.chunk_user = np.asarray(dataload.train_feat["user_id"], dtype=np.int64)
        self.chunk = np.repeat(np.arange(len(lens), dtype=np.int64), lens)                    # chunk of each sample
        within = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
        self.col = (W - lens)[self.chunk] + within                                            # column of the sample's positive
        self._set_units(len(self.chunk))
        if self.item_num <= 2:
            raise ValueError("SampleAcfTrainBatcher: no negative can be drawn from [1, item_num) outside a chunk")

    def make_batch(self, rows, rng):
        win, col = self.windows[self.chunk[rows]], self.col[rows]          # [B, L+1], [B]
        B, W = win.shape
        k = np.arange(W - 1, dtype=np.int64)[None, :]
        profile = np.take_along_axis(win, k + (k >= col[:, None]), axis=1)  # the window without column col
        pos = win[np.arange(B), col]
        neg = rng.integers(1, self.item_num, size=B)
        redraw_clashes(neg, _in_row(win), rng, self.item_num, bound=1000, who="SampleAcfTrainBatcher: a chunk")
        return profile, np.stack((pos, neg, self.chunk_user[self.chunk[rows]]), axis=1)


class DinTrainBatcher(SampleAcfTrainBatcher):
    """Vectorised SampleTwoTowerTrainDataset (reference REC/data/dataset/trainset.py:294-332): SampleAcfTrainBatcher's leave-one-out
    samples without the user id.  Every position j of every SEQ chunk is one sample: profile = the chunk without item j (order
    kept, left-padded with 0 to L), positive = item j, one negative uniform over [1, item_num - 1] and redrawn while it lies in
    the chunk.  The reference stacks a chunk's samples into one dataset item, so its batches hold `train_batch_size` chunks; here
    a batch holds `train_batch_size` samples (ACF's decision).  Yields whole (profile int64 [B, L], target int64 [B, 2] =
    (positive, negative)) batches: the two tensors the training loop stages (DIN.forward joins them into the reference's
    [B, L + 2] row)."""

    def make_batch(self, rows, rng):
        profile, tail = super().make_batch(rows, rng)
        return profile, np.ascontiguousarray(tail[:, :2])


def positions_into_distinct_images(profile, target):
    """(profile [S, L], target [S, 2]) item ids -> (index int64 [S, L + 2] = [profile | positive | negative], image_ids int64 [M]):
    image_ids[0] == 0 (the zero image, "no item"), image_ids[1:] the batch's distinct item ids, ascending; `index` holds positions
    into image_ids."""
    items = np.concatenate((profile, target), axis=1)
    uniq = np.unique(items)
    image_ids = np.concatenate((np.zeros(1, dtype=np.int64), uniq[uniq != 0]))
    return np.searchsorted(image_ids, items), image_ids


def positions_into_distinct_images_masked(items, mask_token):
    """BERT4Rec's items [B, 3, P] (masked sequence | original sequence | negatives; `mask_token` = item_num where a position is
    masked) -> (index int64 [B, 3, P], image_ids int64 [M]): image_ids[0] == 0 (the zero image, "no item"), image_ids[1] ==
    mask_token (it stands for the ones image, which no store holds), image_ids[2:] the batch's other distinct item ids, ascending;
    `index` holds positions into image_ids.  The two leading rows are there whether or not the batch reads them."""
    uniq = np.unique(items)
    image_ids = np.concatenate((np.asarray([0, mask_token], dtype=np.int64), uniq[(uniq != 0) & (uniq != mask_token)]))
    index = 2 + np.searchsorted(image_ids[2:], items)
    index = np.where(items == 0, 0, np.where(items == mask_token, 1, index))
    return index.astype(np.int64), image_ids


class MoPoolTrainBatcher(DinTrainBatcher):
    """Vectorised MOSampleTwoTowerTrainDataset / MOSampleOneTowerTrainDataset + mosampletower_train_collate (reference
    REC/data/dataset/trainset.py:656-813, collate_fn.py:95-107) for MODSSM and MOFM.  A batch is `train_batch_size` whole SEQ chunks
    -- the reference's batch unit -- so the frame's order and rank split run over chunks; every position of every chunk is one
    leave-one-out sample, formed by DinTrainBatcher.make_batch over the chunks' samples in chunk order (profile = the chunk without
    the item, order kept, left-padded; one negative outside the chunk), so S = the sum of the chunk lengths.

    Yields (index int64 [S, L + 2] = [profile | positive | negative], image_ids int64 [M]): image_ids[0] == 0 (the zero image,
    "no item"), image_ids[1:] the batch's distinct item ids, ascending; `index` holds positions into image_ids.  Each distinct
    image is therefore fetched and encoded ONCE per batch.  The reference lists 1 + 2 n images per chunk of n items and so
    dedups inside a chunk only; here the dedup runs across the whole batch.  The CLIP tower is a per-image function without batch
    statistics or dropout, so an image encoded once and read by several chunks receives the sum of the gradients its copies
    would have received: the same parameter gradients."""

    def __init__(self, config, dataload, rank=0, world=1, seed=0, drop_last=False):
        super().__init__(config, dataload, rank=rank, world=world, seed=seed, drop_last=drop_last)
        self.first = np.cumsum(self.lens) - self.lens                 # first sample of each chunk
        self.n_samples = self.n
        self._set_units(len(self.windows))                            # the unit of the order and of a batch: the chunk

    def make_batch(self, chunks, rng):
        lens = self.lens[chunks]
        rows = np.repeat(self.first[chunks] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()), dtype=np.int64)
        return positions_into_distinct_images(*super().make_batch(rows, rng))


class CuratorTrainBatcher(TrainBatcher):
    """Vectorised TwoTowerTrainDataset (reference REC/data/dataset/trainset.py:256-290) over the SEQ chunks.  The reference maps
    CuratorNet to a `TwoTowerTrainDataset2` that does not exist (REC/data/utils.py:39); CuratorNet.forward reads [profile |
    positive | negative] rows, which is TwoTowerTrainDataset's row format, and the class is InputType.SEQ, so Data builds the
    chunks of at most L+1 items.  One sample per chunk: profile = the chunk without its last item, left-padded with 0 to L;
    positive = the last item; one negative uniform over [1, item_num - 1] and redrawn while it lies in the chunk -- the
    reference's distribution, not its random stream.  A chunk of one item gives an all-padding profile.  Yields whole (profile
    int64 [B, L], target int64 [B, 2] = (positive, negative)) batches: the two tensors the training loop stages
    (CuratorNet.forward joins them into the [B, L + 2] row)."""

    def __init__(self, config, dataload, rank=0, world=1, seed=0, drop_last=False):
        super().__init__(config, dataload, rank=rank, world=world, seed=seed, drop_last=drop_last)
        self.L = config["MAX_ITEM_LIST_LENGTH"]
        self.windows, _ = left_padded_windows(dataload.train_feat["item_seq"], self.L + 1)    # the chunks
        self._set_units(len(self.windows))
        if self.item_num <= 2:
            raise ValueError("CuratorTrainBatcher: no negative can be drawn from [1, item_num) outside a chunk")

    def make_batch(self, rows, rng):
        win = self.windows[rows]                                       # [B, L+1]
        neg = rng.integers(1, self.item_num, size=len(win))
        redraw_clashes(neg, _in_row(win), rng, self.item_num, bound=1000, who="CuratorTrainBatcher: a chunk")
        return win[:, :-1].copy(), np.stack((win[:, -1], neg), axis=1)


class MoTowerTrainBatcher(CuratorTrainBatcher):
    """Vectorised MOTwoTowerTrainDataset (reference REC/data/utils.py:44 maps MODIN to it) over the SEQ chunks: CuratorTrainBatcher's
    samples -- one per chunk: the chunk without its last item is the profile, the last item the positive, one negative outside the
    chunk -- as positions into the batch's distinct images.  The reference's dataset returns the images alone while
    MODIN.forward unpacks (items_modal, items); here the batcher carries the ids.

    Yields (index int64 [B, L + 2] = [profile | positive | negative], image_ids int64 [M]) with MoPoolTrainBatcher's batch-wide
    dedup: image_ids[0] == 0 (the zero image, "no item"), image_ids[1:] the batch's distinct item ids, ascending; `index` holds
    positions into image_ids, so each distinct image is fetched and encoded once per batch."""

    def make_batch(self, rows, rng):
        return positions_into_distinct_images(*super().make_batch(rows, rng))


class MoBert4RecTrainBatcher(BERT4RecTrainBatcher):
    """Vectorised MOBERT4RecTrainDataset (reference REC/data/dataset/trainset.py:836-935) for MOBERT4Rec: BERT4RecTrainBatcher's
    batches -- the same windows, masking, negatives and random stream -- as positions into the batch's distinct images.

    Yields (index int64 [B, 3, L+1], masked_index int64 [B, L+1], image_ids int64 [M]): image_ids[index] is
    BERT4RecTrainBatcher's `items`; image_ids[0] == 0 (the zero image), image_ids[1] == item_num (the mask token: the ones image),
    image_ids[2:] the batch's other distinct ids, ascending.  The reference lists one image per (position, input | positive |
    negative): 3 B (L+1) per batch; here each distinct image is fetched and encoded once.  It feeds the ones image at padded
    input positions too (trainset.py:907); those are masked keys outside the loss, so they hold position 0 here -- the same loss
    and the same gradients (README "MOBERT4Rec")."""

    def make_batch(self, rows, rng):
        items, masked = super().make_batch(rows, rng)
        index, image_ids = positions_into_distinct_images_masked(items, self.mask_token)
        return index, masked, image_ids


class PairTrainBatcher(TrainBatcher):
    """Vectorised PairTrainDataset (reference REC/data/dataset/trainset.py:171-198): one sample per training interaction, yielded
    as whole (user int64 [B], item int64 [B, 2] = (positive, negative)) batches.  The negative is uniform over [1, item_num - 1]
    and redrawn while it lies in the user's training history user_seq[user][:-2] -- the reference's distribution, not its random
    stream."""

    def __init__(self, config, dataload, rank=0, world=1, seed=0, drop_last=False):
        super().__init__(config, dataload, rank=rank, world=world, seed=seed, drop_last=drop_last)
        self.users = np.asarray(dataload.train_feat["user_id"], dtype=np.int64)
        self.items = np.asarray(dataload.train_feat["item_id"], dtype=np.int64)
        self._set_units(len(self.users))
        # membership keys user * item_num + item of every training interaction (= every user's user_seq[:-2]), sorted
        self._keys = np.unique(self.users * self.item_num + self.items)
        # a user whose history covers every candidate would loop forever in the reference: refuse up front
        hist = np.bincount(self._keys // self.item_num)
        if self.item_num <= 1 or (hist >= self.item_num - 1).any():
            raise ValueError("PairTrainBatcher: a user has interacted with every item: no negative can be drawn")

    def in_history(self, user, item):
        """bool array: item[k] is in user[k]'s training history."""
        keys = user * self.item_num + item
        pos = np.minimum(np.searchsorted(self._keys, keys), len(self._keys) - 1)
        return self._keys[pos] == keys

    def make_batch(self, rows, rng):
        user = self.users[rows]
        neg = rng.integers(1, self.item_num, size=len(rows))
        # no limit: the constructor has refused every user without a candidate, so each round ends with probability > 0
        redraw_clashes(neg, lambda neg: self.in_history(user, neg), rng, self.item_num, bound=None, who=None)
        return user, np.stack((self.items[rows], neg), axis=1)


def positions_into_distinct_items(item):
    """item [B, 2] item ids (positive, negative) -> (index int64 [B, 2], image_ids int64 [M]): image_ids the batch's distinct item
    ids, ascending, WITHOUT a zero image in front (a pair model has no padding position); `index` holds positions into image_ids,
    base 0, so image_ids[index] == item."""
    image_ids, index = np.unique(item, return_inverse=True)
    return index.reshape(item.shape).astype(np.int64), image_ids.astype(np.int64)


class MoPairTrainBatcher(PairTrainBatcher):
    """Vectorised MOPairTrainDataset (reference REC/data/dataset/trainset.py:202; REC/data/utils.py:42 maps MOMF to it) for MOMF:
    PairTrainBatcher's batches -- the same users, positives, negatives and random stream -- with the items as positions into the
    batch's distinct images.

    Yields (user int64 [B], index int64 [B, 2], image_ids int64 [M]): image_ids[index] is PairTrainBatcher's `item`; image_ids is
    the batch's distinct item ids, ascending, M <= 2B.  There is no zero image in front: MOMF has no padding position, and a
    33rd image at B = 16 would be 3 % more tower work for a row nothing reads.  The reference stacks one image per (sample,
    positive | negative), 2B per batch; here each distinct image is fetched and encoded once."""

    def make_batch(self, rows, rng):
        user, item = super().make_batch(rows, rng)
        index, image_ids = positions_into_distinct_items(item)
        return user, index, image_ids


class GraphTrainBatcher(TrainBatcher):
    """Vectorised GraphTrainDataset (reference REC/data/dataset/trainset.py:939-981): one sample per AUGSEQ prefix
    (Data._build_aug_seq), yielded as whole (item_seq int64 [B, L], mask int64 [B, L], target int64 [B, 2]) batches.  item_seq =
    prefix[:-1] RIGHT-padded with 0, mask = 1 on its real positions, target = (prefix[-1], negative); the negative is uniform
    over [1, item_num - 1] and redrawn while it lies in the prefix -- the reference's distribution, not its random stream."""

    def __init__(self, config, dataload, rank=0, world=1, seed=0, drop_last=False):
        super().__init__(config, dataload, rank=rank, world=world, seed=seed, drop_last=drop_last)
        self.L = config["MAX_ITEM_LIST_LENGTH"]
        self.flat = np.asarray(dataload._sorted_items, dtype=np.int64)
        self.start = np.asarray(dataload.train_feat["seq_start"], dtype=np.int64)
        self.length = np.asarray(dataload.train_feat["seq_len"], dtype=np.int64)
        self._set_units(len(self.start))
        if self.item_num <= 2:
            raise ValueError("GraphTrainBatcher: no negative can be drawn from [1, item_num) outside a prefix")

    def make_batch(self, rows, rng):
        st, ln = self.start[rows], self.length[rows]
        B, L = len(rows), self.L
        win = gather_windows(self.flat, st, ln, L + 1, left_pad=False)     # [B, L+1]: the prefix, target included
        real = np.arange(L, dtype=np.int64)[None, :] < (ln - 1)[:, None]
        item_seq = np.where(real, win[:, :L], 0)
        pos = win[np.arange(B), ln - 1]
        neg = rng.integers(1, self.item_num, size=B)
        redraw_clashes(neg, _in_row(win), rng, self.item_num, bound=1000, who="GraphTrainBatcher: a prefix")
        return item_seq, real.astype(np.int64), np.stack((pos, neg), axis=1)


class MoGraphTrainBatcher(GraphTrainBatcher):
    """Vectorised MOGraphTrainDataset + mograph_train_collate (reference REC/data/dataset/trainset.py, collate_fn.py) for MOSRGNN:
    GraphTrainBatcher's batches -- the same AUGSEQ prefixes, negatives and random stream -- as positions into the batch's distinct
    images.  The mask is not carried: the prefixes are right-padded, so it is index != 0 and the graph build derives it.

    Yields (index int64 [B, L + 2] = [item_seq | positive | negative], image_ids int64 [M]): image_ids[index] is
    GraphTrainBatcher's [item_seq | target]; image_ids[0] == 0 (the zero image, "no item"), image_ids[1:] the batch's distinct item
    ids, ascending -- so a session's node order by position is its node order by id, np.unique's order in the reference collate.
    The reference stacks one image per node slot and target, B (n + 2) per batch with n the batch's largest node count, pad images
    included; here each distinct image is fetched and encoded once.  The batch unit stays the reference's: `train_batch_size`
    shuffled prefixes (README "MOSRGNN")."""

    def make_batch(self, rows, rng):
        item_seq, _, target = super().make_batch(rows, rng)
        return positions_into_distinct_images(item_seq, target)


class _NoTraining:
    """The train side of a model that is not trained (VISRANK): a `_TrainLoader`-shaped object without batches."""

    def __init__(self, dataload):
        self.dataload = dataload
        self.item_num = dataload.item_num
        self.batcher = self.sampler = self.dataset = self

    def set_epoch(self, epoch):
        return None

    def __len__(self):
        return 0

    def __iter__(self):
        return iter(())


class SeqEvalBatcher:
    """Vectorised equivalent of DataLoader(SeqEvalDataset, sampler=NonConsecutiveSequentialDistributedSampler,
    collate_fn=seq_eval_collate) (reference evalset.py:4-36, collate_fn.py:6-32, data/utils.py:134-159): yields the same
    `(item_seq [b,L], (history_u, history_i), positive_u [b], item_target [b])` batches, built from a CSR image of the
    user sequences with numpy index arithmetic instead of one Python __getitem__ per user (200 K users: 1.6 s -> ms).
    Duck-types what the Trainer reads from a DataLoader: iteration, `len()`, `.dataset.dataload`, `.sampler.dataset`.
    A subclass overrides model_input() -- the batch's first element -- and nothing else."""

    def __init__(self, config, dataload, phase="valid", rank=0, world=1):
        self.dataset = SeqEvalDataset(config, dataload, phase=phase)       # keeps the per-user API (and the tests) alive
        self.sampler = type("Sampler", (), {"dataset": self.dataset})()
        self.batch_size = config["eval_batch_size"]
        self.L = config["MAX_ITEM_LIST_LENGTH"]
        seqs = self.dataset.user_seq
        lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
        self.offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
        np.cumsum(lens, out=self.offsets[1:])
        self.flat = np.concatenate([np.asarray(s, dtype=np.int64) for s in seqs]) if len(seqs) else np.zeros(0, np.int64)
        self.cut = lens - (2 if phase == "valid" else 1)                   # history = seq[:cut], target = seq[cut]
        self.users = np.arange(rank, len(seqs), world, dtype=np.int64)     # rank r takes users r, r+W, ... (no padding)

    def __len__(self):
        return -(-len(self.users) // self.batch_size)

    @functools.cached_property
    def uids(self):
        """The user id (the key of user_seq) of every user index."""
        user_seq = self.dataset.dataload.user_seq
        return np.fromiter(user_seq.keys(), dtype=np.int64, count=len(user_seq))

    def model_input(self, u, start, cut):
        """The first element of a batch, as numpy, for the user indices u [b] with history flat[start : start + cut]: here the
        last L history items, left-padded with 0."""
        return gather_windows(self.flat, start, cut, self.L, left_pad=True)

    def __iter__(self):
        for b0 in range(0, len(self.users), self.batch_size):
            u = self.users[b0:b0 + self.batch_size]
            start, cut = self.offsets[u], self.cut[u]
            target = self.flat[start + cut]
            # history pairs (row in batch, item) for every past interaction
            hist_u = np.repeat(np.arange(len(u), dtype=np.int64), cut)
            first = np.cumsum(cut) - cut                                   # first pair of each user
            hist_i = self.flat[np.repeat(start - first, cut) + np.arange(len(hist_u), dtype=np.int64)]
            yield (torch.from_numpy(self.model_input(u, start, cut)), (torch.from_numpy(hist_u), torch.from_numpy(hist_i)),
                   torch.arange(len(u)), torch.from_numpy(target))


class PairEvalBatcher(SeqEvalBatcher):
    """PairEvalDataset (reference evalset.py:41-66) through SeqEvalBatcher: the same users, histories and targets (valid:
    [:-2] / [-2], test: [:-1] / [-1]), with the user ids in place of the item windows:
    `(user [b], (history_u, history_i), positive_u [b], item_target [b])`."""

    def model_input(self, u, start, cut):
        return self.uids[u]


class AcfEvalBatcher(SeqEvalBatcher):
    """ACFEvalDataset (reference evalset.py) through SeqEvalBatcher: the same users, windows, histories and targets, with the
    user id (the key of user_seq) appended to the window as column L:
    `([item_seq | user id] [b, L + 1], (history_u, history_i), positive_u [b], item_target [b])`."""

    def model_input(self, u, start, cut):
        return np.concatenate((super().model_input(u, start, cut), self.uids[u][:, None]), axis=1)


class VisRankEvalBatcher(SeqEvalBatcher):
    """VisRankEvalDataset (reference evalset.py:113-145; one unpadded history per batch of 1) through SeqEvalBatcher: the same users,
    targets and FULL-history pairs, with the model's window -- the last `history_window` history items (visrank.py:39 user[-50:],
    default 50), left-padded with 0 -- in place of the MAX_ITEM_LIST_LENGTH window:
    `(window [b, history_window], (history_u, history_i), positive_u [b], item_target [b])`."""

    def __init__(self, config, dataload, phase="valid", rank=0, world=1):
        super().__init__(config, dataload, phase=phase, rank=rank, world=world)
        w = config["history_window"] if "history_window" in config else None
        self.L = 50 if w is None else int(w)
        if (self.cut < 1).any():
            raise ValueError("VisRankEvalBatcher: a user without history (the mean of nothing)")


class GraphEvalBatcher(SeqEvalBatcher):
    """GraphEvalDataset (reference evalset.py:187-224) through SeqEvalBatcher: the same users, histories and targets, with the
    last L history items RIGHT-padded with 0 (the sequence models' batcher left-pads).  The mask of a right-padded window is
    item_seq != 0; the model derives it on the device.  `(item_seq [b, L], (history_u, history_i), positive_u [b], target [b])`."""

    def model_input(self, u, start, cut):
        n = np.minimum(cut, self.L)
        return gather_windows(self.flat, start + cut - n, n, self.L, left_pad=False)


