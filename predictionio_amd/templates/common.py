"""Shared template helpers: device-resident query filters.

The reference's isCandidateItem filters (similarproduct
ALSAlgorithm.scala:245-271, ecommerce ECommAlgorithm.scala:330-430)
re-scan the item metadata dict per query. Here category membership is
precomputed ONCE at train time as per-category uint8 device masks, so
query-time category filtering is a handful of tensor ops — flat in
catalog size. `CategoryBits` packs the same
membership into per-item bit words, so a whole batch of differently
filtered queries runs as one fused top-K launch."""

from __future__ import annotations

from typing import Dict, Iterable, List, Optional

import torch


class CategoryMasks:
    """Per-category item-membership masks (uint8, 1 = member)."""

    def __init__(self, masks: Dict[str, torch.Tensor], n: int, device):
        self.masks = masks
        self.n = n
        self.device = device

    @classmethod
    def build(cls, items: Dict[str, object], item_map,
              device) -> "CategoryMasks":
        """items: item-id → metadata with a `.categories` list."""
        masks: Dict[str, torch.Tensor] = {}
        n = len(item_map)
        for it, meta in items.items():
            cats = getattr(meta, "categories", None) or []
            if not cats:
                continue
            i = item_map.get(it)
            if i is None:
                continue
            for c in cats:
                m = masks.get(c)
                if m is None:
                    m = torch.zeros(n, dtype=torch.uint8)
                    masks[c] = m
                m[i] = 1
        return cls({c: m.to(device) for c, m in masks.items()}, n, device)

    def banned_outside(self, categories: Iterable[str]) -> torch.Tensor:
        """uint8 mask with 1 for items NOT in any given category — the
        ban contribution of a query's `categories` filter."""
        allowed: Optional[torch.Tensor] = None
        for c in categories:
            m = self.masks.get(c)
            if m is not None:
                allowed = m if allowed is None else (allowed | m)
        if allowed is None:
            return torch.ones(self.n, dtype=torch.uint8,
                              device=self.device)
        return 1 - allowed


class CategoryBits:
    """Per-item category bit words for the fused kernels' per-query
    filter (`topk_score(..., item_cats=, query_cats=)`).

    Bit 0 of word 0 is an ANY bit set on every item; category c owns bit
    1 + ordinal(c) (ordinal = order of first appearance at build time).
    W is the smallest of {1, 2, 4} 32-bit words that holds all bits, so
    at most 127 categories fit. Words are assembled as numpy uint32 and
    viewed as int32 — bit 31 is an ordinary category bit."""

    MAX_CATEGORIES = 127

    def __init__(self, ordinals: Dict[str, int], item_words: torch.Tensor):
        self.ordinals = ordinals
        self.item_words = item_words          # [N, W] int32, on device
        self.W = int(item_words.shape[1])

    @classmethod
    def build(cls, items: Dict[str, object], item_map,
              device) -> Optional["CategoryBits"]:
        """items: item-id → metadata with a `.categories` list. Returns
        None when the catalog has more than 127 categories (the caller
        then keeps the per-query CategoryMasks path)."""
        import numpy as np
        ordinals: Dict[str, int] = {}
        member: List[tuple] = []              # (item index, ordinal)
        for it, meta in items.items():
            cats = getattr(meta, "categories", None) or []
            if not cats:
                continue
            i = item_map.get(it)
            if i is None:
                continue
            for c in cats:
                o = ordinals.get(c)
                if o is None:
                    o = len(ordinals)
                    if o >= cls.MAX_CATEGORIES:
                        return None
                    ordinals[c] = o
                member.append((i, o))
        nbits = 1 + len(ordinals)
        W = 1 if nbits <= 32 else 2 if nbits <= 64 else 4
        words = np.zeros((len(item_map), W), dtype=np.uint32)
        words[:, 0] = 1                       # ANY bit
        if member:
            idx = np.asarray(member, dtype=np.int64)
            bit = idx[:, 1] + 1
            np.bitwise_or.at(
                words, (idx[:, 0], bit >> 5),
                np.left_shift(np.uint32(1), (bit & 31).astype(np.uint32)))
        return cls(ordinals,
                   torch.from_numpy(words.view(np.int32)).to(device))

    def query_words(self, categories: Optional[Iterable[str]]):
        """numpy int32 [W] accepted-category words of one query: None →
        the ANY bit (every item passes); a list → the OR of its known
        categories; no known category (or []) → all zero, so nothing
        passes — what `CategoryMasks.banned_outside` does."""
        import numpy as np
        words = np.zeros(self.W, dtype=np.uint32)
        if categories is None:
            words[0] = 1
        else:
            for c in categories:
                o = self.ordinals.get(c)
                if o is not None:
                    bit = o + 1
                    words[bit >> 5] |= np.uint32(1) << np.uint32(bit & 31)
        return words.view(np.int32)


def ban_csr(ban_lists: List[List[int]], device):
    """Per-query sorted ban lists → the kernels' CSR (int64 indptr,
    int32 indices) on `device`."""
    import numpy as np
    lens = np.fromiter((len(b) for b in ban_lists), dtype=np.int64,
                       count=len(ban_lists))
    indptr = np.zeros(len(ban_lists) + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    flat = np.fromiter((x for b in ban_lists for x in b), dtype=np.int32,
                       count=int(indptr[-1]))
    return (torch.from_numpy(indptr).to(device),
            torch.from_numpy(flat).to(device))


def ids_tensor(ids: Iterable[str], id_map, device) -> torch.Tensor:
    """Map string ids through a BiMap into an int64 index tensor,
    dropping unknowns."""
    idxs: List[int] = []
    for s in ids:
        i = id_map.get(s)
        if i is not None:
            idxs.append(i)
    return torch.tensor(idxs, dtype=torch.int64, device=device)
