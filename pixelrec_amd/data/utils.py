"""load_data / bulid_dataloader with the reference's names (REC/data/utils.py:15-114) for the SASRec family.

Train side: `SeqTrainBatcher` (vectorised whole batches; order = torch DistributedSampler's).  Eval side: the
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
from .dataset import (AcfEvalBatcher, BERT4RecTrainBatcher, CuratorTrainBatcher, DinTrainBatcher, GraphEvalBatcher, GraphTrainBatcher, MoBert4RecTrainBatcher, MoPoolTrainBatcher, MoTowerTrainBatcher, PairEvalBatcher, PairTrainBatcher, SeqEvalBatcher,
                      SampleAcfTrainBatcher, SeqEvalDataset, SeqTrainBatcher, TwoTowerTrainBatcher, VisRankEvalBatcher, _NoTraining,
                      seq_eval_collate)

SUPPORTED = {"SASRec": "SEQ", "MOSASRec": "SEQ", "FSASRec": "SEQ", "GRU4Rec": "SEQ", "NextItNet": "SEQ",
             "MOGRU4Rec": "SEQ", "MONextItNet": "SEQ", "BERT4Rec": "SEQ", "LightGCN": "PAIR", "MF": "PAIR", "VBPR": "PAIR",
             "SRGNN": "AUGSEQ", "LightSANs": "TWOTOWER", "ACF": "SEQ", "VISRANK": "EVALONLY", "CuratorNet": "SEQ", "DIN": "SEQ",
             "DSSM": "SEQ", "FM": "SEQ", "WideDeep": "SEQ", "MODSSM": "SEQ", "MOFM": "SEQ",
             "MODIN": "SEQ", "MOBERT4Rec": "SEQ"}      # REC/data/utils.py:24-33


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
    """DataLoader-shaped facade over SeqTrainBatcher: `.sampler.set_epoch`, `len()`, iteration."""

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
    if SUPPORTED[model_name] == "EVALONLY":
        # BaseDataset / VisRankEvalDataset (REC/data/utils.py:37): nothing to train, windows + full histories to score
        if config["need_training"] is not False:
            raise ValueError(f"{model_name} is not trained: set `need_training: False` (reference ViNet/visrank.yaml)")
        return (_NoTraining(dataload), VisRankEvalBatcher(config, dataload, phase="valid", rank=rank, world=world),
                VisRankEvalBatcher(config, dataload, phase="test", rank=rank, world=world))
    if SUPPORTED[model_name] == "PAIR":
        # PairTrainDataset / PairEvalDataset (REC/data/utils.py:24-31): one sample per training interaction, users scored
        train_loader = _TrainLoader(PairTrainBatcher(config, dataload, rank=rank, world=world))
        return (train_loader, PairEvalBatcher(config, dataload, phase="valid", rank=rank, world=world),
                PairEvalBatcher(config, dataload, phase="test", rank=rank, world=world))
    if SUPPORTED[model_name] == "AUGSEQ":
        # GraphTrainDataset / GraphEvalDataset (REC/data/utils.py:24-31): every prefix a sample, right-padded windows
        train_loader = _GraphTrainLoader(GraphTrainBatcher(config, dataload, rank=rank, world=world))
        return (train_loader, GraphEvalBatcher(config, dataload, phase="valid", rank=rank, world=world),
                GraphEvalBatcher(config, dataload, phase="test", rank=rank, world=world))
    # BERT4Rec masks its windows (REC/data/utils.py:25: BERT4RecTrainDataset); LightSANs (AUGSEQ, so Data built every prefix)
    # reads TwoTowerTrainDataset's rows of those prefixes (:35); CuratorNet (:39 names a TwoTowerTrainDataset2 that does not exist)
    # reads the same row format over the SEQ chunks; DIN and DSSM (:31-32 SampleTwoTowerTrainDataset) and FM (:33
    # SampleOneTowerTrainDataset: the same samples as [profile | positive], [profile | negative] planes) read ACF's leave-one-out
    # samples without the user id -- a batch is `train_batch_size` samples (ACF's decision) where the reference stacks
    # `train_batch_size` chunks; evaluation is SeqEvalDataset's for all of them (DIN: CandiEvalDataset's per-item repetition happens
    # inside the kernel); MODSSM and MOFM (MOSampleTwoTowerTrainDataset / MOSampleOneTowerTrainDataset) read the same samples by
    # whole chunks, as positions into the batch's distinct images (MoPoolTrainBatcher); MODIN (:44 MOTwoTowerTrainDataset) reads
    # CuratorNet's one sample per chunk in the same positional form (MoTowerTrainBatcher); MOBERT4Rec (:48 MOBERT4RecTrainDataset)
    # reads BERT4Rec's masked windows in that form, the mask token standing for the ones image (MoBert4RecTrainBatcher)
    batcher = {"BERT4Rec": BERT4RecTrainBatcher, "LightSANs": TwoTowerTrainBatcher,
               "ACF": SampleAcfTrainBatcher, "CuratorNet": CuratorTrainBatcher, "DIN": DinTrainBatcher, "DSSM": DinTrainBatcher,
               "FM": DinTrainBatcher, "WideDeep": CuratorTrainBatcher, "MODSSM": MoPoolTrainBatcher,
               "MOFM": MoPoolTrainBatcher, "MODIN": MoTowerTrainBatcher, "MOBERT4Rec": MoBert4RecTrainBatcher}.get(model_name, SeqTrainBatcher)
    train_loader = _TrainLoader(batcher(config, dataload, rank=rank, world=world))
    if model_name == "ACF":
        # SampleACFTrainDataset / ACFEvalDataset (REC/data/utils.py:24-31): leave-one-out samples of the chunks; windows + user id
        return (train_loader, AcfEvalBatcher(config, dataload, phase="valid", rank=rank, world=world),
                AcfEvalBatcher(config, dataload, phase="test", rank=rank, world=world))
    loaders = []
    workers = int(config["eval_num_workers"] or 0)
    for phase in ("valid", "test"):
        if config["eval_vectorized"] is None or bool(config["eval_vectorized"]):
            loaders.append(SeqEvalBatcher(config, dataload, phase=phase, rank=rank, world=world))
            continue
        # literal form of the reference's loaders (data/utils.py:95-110); `eval_vectorized: False` selects it
        ds = SeqEvalDataset(config, dataload, phase=phase)
        sampler = NonConsecutiveSequentialDistributedSampler(ds, rank=rank, num_replicas=world)
        loaders.append(DataLoader(ds, batch_size=config["eval_batch_size"], num_workers=workers, pin_memory=False,
                                  sampler=sampler, collate_fn=seq_eval_collate))
    return train_loader, loaders[0], loaders[1]
