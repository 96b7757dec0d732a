"""Data -- interaction CSV -> per-user sequences -> training windows, with the reference's exact rules
(code/REC/data/dataload.py) but vectorised (the reference walks Python dict/list loops, dataload.py:94-150).

Wire format: `<data_path>/<dataset>.csv`, header row, columns item_id,user_id,timestamp (dataload.py:30-37).
Ids are factorised in first-appearance (file) order, +1, 0 = '[PAD]' (:46-54).  build(): sort by timestamp
(pandas sort_values, :68), group per user keeping time order (:71-77), train = all but the last two
interactions of each user (:80-83), then windows of MAX_ITEM_LIST_LENGTH+1: a longer history drops its OLDEST
`len % (L+1)` items and is cut into consecutive full windows, a shorter one is a single window (:103-150).
"""
from __future__ import annotations

import os
from logging import getLogger

import numpy as np
import pandas as pd

from ..utils.enum_type import InputType


class Data:
    def __init__(self, config):
        self.config = config
        self.dataset_path = config["data_path"]
        self.dataset_name = config["dataset"]
        self.logger = getLogger()
        self._load_inter_feat(self.dataset_name, self.dataset_path)
        self._data_processing()

    def _load_inter_feat(self, token, dataset_path):
        path = os.path.join(dataset_path, f"{token}.csv")
        if not os.path.isfile(path):
            raise ValueError(f"File {path} not exist.")
        self.inter_feat = pd.read_csv(path, delimiter=",", dtype={"item_id": str, "user_id": str, "timestamp": int},
                                      header=0, names=["item_id", "user_id", "timestamp"])

    def _data_processing(self):
        self.id2token, self.token2id = {}, {}
        for feature in ["user_id", "item_id"]:
            new_ids, mp = pd.factorize(self.inter_feat[feature])
            mp = np.array(["[PAD]"] + list(mp))
            self.id2token[feature] = mp
            self.token2id[feature] = {t: i for i, t in enumerate(mp)}
            self.inter_feat[feature] = new_ids + 1
        self.user_num = len(self.id2token["user_id"])
        self.item_num = len(self.id2token["item_id"])
        self.inter_num = len(self.inter_feat)
        self.uid_field, self.iid_field = "user_id", "item_id"
        self.user_seq = None
        self.train_feat = None

    def build(self):
        self.inter_feat.sort_values(by="timestamp", ascending=True, inplace=True)
        users = self.inter_feat["user_id"].values
        items = self.inter_feat["item_id"].values
        # group by user in first-appearance order, keeping time order inside each group
        uniq, first_pos, inv = np.unique(users, return_index=True, return_inverse=True)
        order_of_first = np.argsort(first_pos, kind="stable")          # users ranked by first appearance
        rank_of_user = np.empty_like(order_of_first)
        rank_of_user[order_of_first] = np.arange(len(uniq))
        grp = rank_of_user[inv]                                         # group id per interaction
        perm = np.argsort(grp, kind="stable")                           # stable => time order inside a group
        counts = np.bincount(grp, minlength=len(uniq))
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
        sorted_items = items[perm]
        uids = uniq[order_of_first]
        self.user_seq = {int(uids[g]): sorted_items[starts[g]:starts[g] + counts[g]] for g in range(len(uniq))}
        self._uids, self._starts, self._counts, self._sorted_items = uids, starts, counts, sorted_items

        if self.config["MODEL_INPUT_TYPE"] == InputType.PAIR:
            self.train_feat = self._build_pair()
            return
        if self.config["MODEL_INPUT_TYPE"] == InputType.AUGSEQ:
            self.train_feat = self._build_aug_seq()
            return
        if self.config["MODEL_INPUT_TYPE"] not in (InputType.SEQ, None):
            raise NotImplementedError("only InputType.SEQ (SASRec family), InputType.PAIR (LightGCN) and InputType.AUGSEQ (SRGNN) "
                                      "are built on this path")
        self.train_feat = self._build_seq()

    def _build_pair(self):
        """dataload.py:80-83 without the window step: every user's interactions but the last two, users in first-appearance
        order, time order inside a user -- one (user, item) training pair each."""
        keep = np.maximum(self._counts - 2, 0)
        first = np.repeat(self._starts, keep)
        within = np.arange(int(keep.sum()), dtype=np.int64) - np.repeat(np.cumsum(keep) - keep, keep)
        return {"user_id": np.repeat(self._uids, keep).astype(np.int64),
                "item_id": self._sorted_items[first + within].astype(np.int64)}

    def get_norm_adj_csr(self):
        """The normalised graph of dataload.py:318-339 as CSR (row_ptr int64, col int32, w fp32): see norm_adj_csr."""
        return norm_adj_csr(self.train_feat[self.uid_field], self.train_feat[self.iid_field], self.user_num, self.item_num)

    def _build_seq(self):
        W = self.config["MAX_ITEM_LIST_LENGTH"] + 1
        uid_list, seqs = [], []
        for g in range(len(self._uids)):
            n = int(self._counts[g]) - 2          # leave-last-two-out
            if n <= 0:
                continue
            s = int(self._starts[g])
            hist = self._sorted_items[s:s + n]
            if n > W:
                off = n % W
                for c in range((n - off) // W):
                    uid_list.append(self._uids[g])
                    seqs.append(hist[off + c * W: off + (c + 1) * W])
            else:
                uid_list.append(self._uids[g])
                seqs.append(hist)
        return {"user_id": np.array(uid_list), "item_seq": seqs}

    def _build_aug_seq(self):
        """dataload.py:152-200: the chunks of _build_seq (at most L+1 items; a longer history drops its oldest len % (L+1)), and
        every prefix of a chunk of length >= 2 is one sample -- chunk order, shorter prefixes first.  Held as index arithmetic
        into the time-ordered item array instead of one list per sample: seq_start (first item of the chunk in
        `self._sorted_items`) and seq_len (prefix length: the history plus its target)."""
        W = self.config["MAX_ITEM_LIST_LENGTH"] + 1
        n = self._counts - 2                                           # leave-last-two-out
        keep = n > 0
        n, s, uid = n[keep], self._starts[keep], self._uids[keep]
        long = n > W
        n_chunks = np.where(long, n // W, 1)
        off = np.where(long, n % W, 0)
        g = np.repeat(np.arange(len(n)), n_chunks)                     # user of each chunk
        c = np.arange(int(n_chunks.sum()), dtype=np.int64) - np.repeat(np.cumsum(n_chunks) - n_chunks, n_chunks)
        c_start = s[g] + off[g] + c * W
        c_len = np.where(long[g], W, n[g])
        per = c_len - 1                                                # prefixes of length 2..len
        k = np.repeat(np.arange(len(c_len)), per)
        within = np.arange(int(per.sum()), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)
        return {"user_id": uid[g][k].astype(np.int64), "seq_start": c_start[k].astype(np.int64),
                "seq_len": (within + 2).astype(np.int64)}

    def aug_item_seqs(self):
        """The AUGSEQ samples as the reference's list of arrays (train_feat['item_seq'] of dataload.py:198): tests / tools."""
        tf = self.train_feat
        return [self._sorted_items[a:a + n] for a, n in zip(tf["seq_start"], tf["seq_len"])]

    # ---- statistics used in the log line -----------------------------------------------------------------
    @property
    def sparsity(self):
        return 1 - self.inter_num / self.user_num / self.item_num

    def __str__(self):
        return "\n".join([str(self.dataset_name), f"The number of users: {self.user_num}",
                          f"The number of items: {self.item_num}", f"The number of inters: {self.inter_num}",
                          f"The sparsity of the dataset: {self.sparsity * 100}%"])

    __repr__ = __str__


def norm_adj_csr(users, items, user_num: int, item_num: int):
    """get_norm_adj_mat (dataload.py:318-339) as CSR over nodes users 0..U-1, items U..U+I-1: every training pair in both
    directions (duplicates stay separate edges), rows = source nodes, edges of a row in edge_index order;
    w = d_src^-1/2 d_dst^-1/2 with d = edges by source (a degree of 0 counts as 1), in fp32 like the reference's tensors.
    -> (row_ptr int64 [U+I+1], col int32 [2n], w fp32 [2n])."""
    u = np.asarray(users, dtype=np.int64)
    i = np.asarray(items, dtype=np.int64) + user_num
    n = user_num + item_num
    if n >= (1 << 31):
        raise ValueError("norm_adj_csr: more than 2^31 nodes")
    src = np.concatenate([u, i])
    dst = np.concatenate([i, u])
    deg = np.bincount(src, minlength=n).astype(np.float32)
    norm = np.float32(1.0) / np.sqrt(np.where(deg == 0, np.float32(1.0), deg))
    w = norm[src] * norm[dst]
    order = np.argsort(src, kind="stable")
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=row_ptr[1:])
    return row_ptr, dst[order].astype(np.int32), w[order].astype(np.float32)
