"""load_data / bulid_dataloader with the reference's names (REC/data/utils.py:15-114).

Train side: one `TrainBatcher` per model, LOADERS below (vectorised whole batches; order = torch DistributedSampler's).  Eval side: the
reference's NonConsecutiveSequentialDistributedSampler sharding -- rank r takes users r, r+W, r+2W, ... with
no padding (utils.py:126-156) -- over SeqEvalDataset + seq_eval_collate.
"""
from __future__ import annotations

import math
from logging import getLogger

import torch
from torch.utils.data import DataLoader

from ..parallel import world_info
from .dataload import Data
from .dataset import (AcfEvalBatcher, BERT4RecTrainBatcher, CuratorTrainBatcher, DinTrainBatcher, GraphEvalBatcher, GraphTrainBatcher, MoBert4RecTrainBatcher, MoGraphTrainBatcher, MoPairTrainBatcher, MoPoolTrainBatcher, MoTowerTrainBatcher, PairEvalBatcher, PairTrainBatcher, SeqEvalBatcher,
                      SampleAcfTrainBatcher, SeqEvalDataset, SeqTrainBatcher, TwoTowerTrainBatcher, VisRankEvalBatcher, _NoTraining,
                      seq_eval_collate)

SUPPORTED = {"SASRec": "SEQ", "MOSASRec": "SEQ", "FSASRec": "SEQ", "GRU4Rec": "SEQ", "NextItNet": "SEQ",
             "MOGRU4Rec": "SEQ", "MONextItNet": "SEQ", "BERT4Rec": "SEQ", "LightGCN": "PAIR", "MF": "PAIR", "VBPR": "PAIR",
             "SRGNN": "AUGSEQ", "LightSANs": "TWOTOWER", "ACF": "SEQ", "VISRANK": "EVALONLY", "CuratorNet": "SEQ", "DIN": "SEQ",
             "DSSM": "SEQ", "FM": "SEQ", "WideDeep": "SEQ", "MODSSM": "SEQ", "MOFM": "SEQ",
             "MODIN": "SEQ", "MOBERT4Rec": "SEQ", "MOSRGNN": "AUGSEQ", "MOMF": "PAIR",
             "DVBPR": "PAIR"}      # REC/data/utils.py:24-33


def load_data(config):
    return Data(config)


class NonConsecutiveSequentialDistributedSampler(torch.utils.data.sampler.Sampler):
    def __init__(self, dataset, rank=None, num_replicas=None):
        r, w = world_info()
        self.dataset = dataset
        self.num_replicas = w if num_replicas is None else num_replicas
        self.rank = r if rank is None else rank
        self.total_size = len(dataset)
        self.num_samples = math.ceil((self.total_size - self.rank) / self.num_replicas)

    def __iter__(self):
        return iter(list(range(self.total_size))[self.rank:self.total_size:self.num_replicas])

    def __len__(self):
        return self.num_samples


class _TrainLoader:
    """DataLoader-shaped facade over a TrainBatcher: `.sampler.set_epoch`, `len()`, iteration."""

    def __init__(self, batcher):
        self.batcher = batcher
        self.sampler = batcher
        self.dataset = batcher
        self.item_num = batcher.item_num

    def __len__(self):
        return len(self.batcher)

    def __iter__(self):
        return iter(self.batcher)


class _GraphTrainLoader(_TrainLoader):
    """GraphTrainBatcher's (item_seq, mask, target) as the two int64 tensors the training loop stages and replays:
    (item_seq [B, L], mask | target [B, L + 2]) -- SRGNN.forward takes either form."""

    def __iter__(self):
        for item_seq, mask, target in self.batcher:
            yield item_seq, torch.cat((mask, target), dim=1)


# model -> (train batcher or None = not trained, eval batcher, train loader facade); on the right the reference's dataset classes
# (REC/data/utils.py:24-48).  A batcher's docstring says how its batches differ from that dataset's.
def _seq_eval(train_batcher):
    return train_batcher, SeqEvalBatcher, _TrainLoader                 # SeqEvalDataset: last-L windows, full histories masked


_SEQ = _seq_eval(SeqTrainBatcher)                                      # SEQTrainDataset: a negative per target position
_POOL = _seq_eval(DinTrainBatcher)                                     # ACF's leave-one-out samples without the user id
_PAIR = (PairTrainBatcher, PairEvalBatcher, _TrainLoader)              # PairTrainDataset / PairEvalDataset: users scored
LOADERS = {
    "SASRec": _SEQ, "MOSASRec": _SEQ, "FSASRec": _SEQ, "GRU4Rec": _SEQ, "NextItNet": _SEQ, "MOGRU4Rec": _SEQ, "MONextItNet": _SEQ,
    "LightGCN": _PAIR, "MF": _PAIR, "VBPR": _PAIR,
    "BERT4Rec": _seq_eval(BERT4RecTrainBatcher),                       # :25 BERT4RecTrainDataset: masked windows
    "SRGNN": (GraphTrainBatcher, GraphEvalBatcher, _GraphTrainLoader),  # Graph{Train,Eval}Dataset: AUGSEQ prefixes, right-padded
    "LightSANs": _seq_eval(TwoTowerTrainBatcher),                      # :35 TwoTowerTrainDataset over the AUGSEQ prefixes
    "ACF": (SampleAcfTrainBatcher, AcfEvalBatcher, _TrainLoader),      # SampleACFTrainDataset / ACFEvalDataset: windows + user id
    "VISRANK": (None, VisRankEvalBatcher, None),                       # :37 BaseDataset / VisRankEvalDataset: nothing to train
    "CuratorNet": _seq_eval(CuratorTrainBatcher),                      # :39 names a TwoTowerTrainDataset2 that does not exist
    "DIN": _POOL,                                                      # :31 SampleTwoTowerTrainDataset; CandiEvalDataset's per-item repetition is the kernel's
    "DSSM": _POOL,                                                     # :32 SampleTwoTowerTrainDataset
    "FM": _POOL,                                                       # :33 SampleOneTowerTrainDataset: the same samples as planes
    "WideDeep": _seq_eval(CuratorTrainBatcher),                        # CuratorNet's one sample per chunk
    "MODSSM": _seq_eval(MoPoolTrainBatcher),                           # MOSampleTwoTowerTrainDataset: DIN's samples by whole chunks
    "MOFM": _seq_eval(MoPoolTrainBatcher),                             # MOSampleOneTowerTrainDataset: the same
    "MODIN": _seq_eval(MoTowerTrainBatcher),                           # :44 MOTwoTowerTrainDataset: CuratorNet's samples
    "MOBERT4Rec": _seq_eval(MoBert4RecTrainBatcher),                   # :48 MOBERT4RecTrainDataset: BERT4Rec's masked windows
    "MOSRGNN": (MoGraphTrainBatcher, GraphEvalBatcher, _TrainLoader),  # :47 MOGraphTrainDataset: SRGNN's AUGSEQ prefixes
    "MOMF": (MoPairTrainBatcher, PairEvalBatcher, _TrainLoader),       # MOPairTrainDataset / PairEvalDataset: MF's pairs, users scored
    "DVBPR": (MoPairTrainBatcher, PairEvalBatcher, _TrainLoader),      # :40 MOPairTrainDataset: the item ids are image_ids[index]
}                                                                      # MO*: as positions into the batch's distinct images
assert LOADERS.keys() == SUPPORTED.keys()


def bulid_dataloader(config, dataload):
    """-> (train_loader, valid_loader, test_loader).  (The misspelt name is the reference's, utils.py:20.)"""
    model_name = config["model"]
    if model_name not in SUPPORTED:
        raise NotImplementedError(f"data pipeline for model {model_name!r} is outside this build's scope")
    dataload.build()
    rank, world = world_info()
    logger = getLogger()
    logger.info(f"[Training]: train_batch_size = [{config['train_batch_size']}]")
    logger.info(f"[Evaluation]: eval_batch_size = [{config['eval_batch_size']}]")
    train_batcher, eval_batcher, facade = LOADERS[model_name]
    if train_batcher is None:
        if config["need_training"] is not False:
            raise ValueError(f"{model_name} is not trained: set `need_training: False` (reference ViNet/visrank.yaml)")
        train_loader = _NoTraining(dataload)
    else:
        train_loader = facade(train_batcher(config, dataload, rank=rank, world=world))
    loaders = []
    for phase in ("valid", "test"):
        if eval_batcher is not SeqEvalBatcher or config["eval_vectorized"] is None or bool(config["eval_vectorized"]):
            loaders.append(eval_batcher(config, dataload, phase=phase, rank=rank, world=world))
            continue
        # literal form of the reference's loaders (data/utils.py:95-110); `eval_vectorized: False` selects it
        ds = SeqEvalDataset(config, dataload, phase=phase)
        sampler = NonConsecutiveSequentialDistributedSampler(ds, rank=rank, num_replicas=world)
        loaders.append(DataLoader(ds, batch_size=config["eval_batch_size"], num_workers=int(config["eval_num_workers"] or 0),
                                  pin_memory=False, sampler=sampler, collate_fn=seq_eval_collate))
    return train_loader, loaders[0], loaders[1]


