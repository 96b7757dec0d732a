"""The frozen ViT prefix kept per item in HBM.

The reference freezes the first `tune_scale` named parameters of the CLIP tower (code/REC/model/load.py:97-99; 165 => blocks 0-9
of 12) and still runs all of them for every image of every step (model/PixelNet/mosasrec.py:69) and for every item of every
evaluation (trainer/trainer.py:339-355).  CLIP has no dropout and the image store applies no augmentation, so the activation that
enters the first trainable block k is a pure function of the item id: `PrefixCache.table[id]` = forward_prefix(store.batch(id)),
[store.n, T*H] fp32 on the store's device.  A training step or an evaluation over item ids then starts at block k
(vit_native.NativeTower.forward_ids; the gather rides in that block's first LayerNorm, pxr_ln_gather_fwd_f32).

Bytes per item = T*H*4: ViT-B/32 153.6 KB, ViT-B/16 605 KB, ViT-L/14 1.05 MB (14.7 / 58.1 / 101 GB for Pixel200K's 96 001 items).

The cache records what it was computed from -- k, the store (its buffer's address and its size) and the tower's flat weight
buffer -- and a use under anything else raises instead of serving rows of another tower or catalogue.
"""
from __future__ import annotations

import logging

import torch

from ..lib import PxrError


def bytes_per_item(T: int, H: int) -> int:
    return T * H * 4


class PrefixCache:
    def __init__(self, table, k, store, flat):
        self.table = table                      # fp32 [store.n, T*H]
        self.k = k                              # the block whose input the rows are
        self.store = store                      # the ImageStore the rows were computed from (callers may re-point it: checked)
        self.store_ptr, self.n = store.images.data_ptr(), store.n
        self.flat_ptr = flat.data_ptr()

    def stale(self, tower, store=None):
        """None, or why the cache may not serve `tower` over `store` (default: the store it holds) now."""
        store = self.store if store is None else store
        k = tower.first_trainable_block()
        if k != self.k:
            return f"the first trainable block is {k}, the cache holds the input of block {self.k}"
        if store.images.data_ptr() != self.store_ptr or store.n != self.n:
            return "the image store is not the one the cache was filled from"
        if tower.flat is None or tower.flat.data_ptr() != self.flat_ptr:
            return "the tower's weights were re-packed since the cache was filled"
        return None

    def check(self, tower) -> int:
        """-> k; PxrError when the cache is stale (host-side: nothing is launched, the status word stays clear)."""
        why = self.stale(tower)
        if why is not None:
            raise PxrError(f"stale prefix cache: {why} (drop_prefix_cache() / build_prefix_cache() again)")
        return self.k


@torch.no_grad()
def build(enc, store, budget_bytes=None, chunk=100):
    """-> a filled PrefixCache of `enc` over `store`, or None (one log line, nothing allocated) when the tower has no frozen
    prefix or the table does not fit `budget_bytes` (default: half of the free device memory -- the fill's own workspace and the
    training step's activations want the rest)."""
    log = logging.getLogger()
    tower = enc._native
    dev = store.images.device
    tower._require_hip(dev)
    tower.ensure_packed()
    k = tower.first_trainable_block()
    if k < 1:
        log.info("prefix cache: not built -- the embeddings or block 0 of the tower train, there is no frozen prefix")
        return None
    H, _, _, T, _ = tower._shape()
    need = store.n * bytes_per_item(T, H)
    if budget_bytes is None:
        budget_bytes = torch.cuda.mem_get_info(dev)[0] // 2
    if need > budget_bytes:
        log.info("prefix cache: not built -- %d items x %d B = %.2f GB exceed the budget of %.2f GB", store.n, bytes_per_item(T, H),
                 need / 1e9, budget_bytes / 1e9)
        return None
    table = torch.empty(store.n, T * H, dtype=torch.float32, device=dev)
    for s in range(0, store.n, chunk):
        e = min(store.n, s + chunk)
        ids = torch.arange(s, e, device=dev)
        # row 0 is the zero image's prefix (not zero); block k-1 writes straight into the table's rows
        tower.forward_prefix(store.batch(ids), out=table[s:e].view(e - s, T, H))
    return PrefixCache(table, k, store, tower.flat)
