"""Oracle for the top-K shortlist contract, and the inputs that probe it.

Pure torch in float64, no GPU and no code from the package under test.

The contract of `topk_score` on the bf16 routes: the candidates that
reach the fp32 re-score contain every valid item whose bf16 score is in
the top D of its query (D = the route's shortlist depth), and the
returned K are the best of the candidates by their fp32 dots. So an item
MUST be returned when it is both in the fp32 top K and in the bf16 top D
by a margin no summation order can undo; nothing else is promised about
the remaining slots except that they hold valid, distinct, correctly
scored items in descending order.

Margins use the project's error-bound form: an fp32-accumulated dot is
within tol[b, j] = f 2^-23 sum_k |x_bk| |y_jk| of the float64 dot (n
roundings of at most 2^-24 relative each, a factor two to spare). Two
scores are "separated" when they differ by more than the sum of their
two bounds.
"""

import torch

NEG_INF = float("-inf")


def bf16_round(t):
    return t.to(torch.bfloat16).double()


def valid_items(B, N, item_mask=None, ban_indptr=None, ban_indices=None,
                item_cats=None, query_cats=None):
    """[B, N] bool: item j passes all of query b's filters."""
    valid = torch.ones((B, N), dtype=torch.bool)
    if item_mask is not None:
        valid &= ~item_mask.bool().unsqueeze(0)
    if ban_indptr is not None:
        ip = ban_indptr.tolist()
        for b in range(B):
            valid[b, ban_indices[ip[b]:ip[b + 1]].long()] = False
    if item_cats is not None:
        hit = torch.zeros((B, N), dtype=torch.bool)
        for w in range(item_cats.shape[1]):
            hit |= (item_cats[:, w].unsqueeze(0)
                    & query_cats[:, w].unsqueeze(1)) != 0
        valid &= hit
    return valid


def _separated_above(score, tol, valid, depth):
    """[B, N] bool: valid items whose score exceeds the (depth+1)-th best
    valid score of their query by more than both error bounds. With
    depth >= n_valid there is no (depth+1)-th: every valid item passes."""
    B, N = score.shape
    masked = score.masked_fill(~valid, NEG_INF)
    out = valid.clone()
    if depth >= N:
        return out
    sv, si = torch.sort(masked, dim=1, descending=True, stable=True)
    cut_v = sv[:, depth]                           # -inf: fewer valid
    cut_t = tol.gather(1, si[:, depth:depth + 1]).squeeze(1)
    has_cut = cut_v > NEG_INF
    sep = (score - cut_v.unsqueeze(1)) > (tol + cut_t.unsqueeze(1))
    return out & (sep | ~has_cut.unsqueeze(1))


class Oracle:
    """Float64 scores, validity and the must-have sets of one problem.
    Build once per (inputs, K, D); never modified afterwards."""

    def __init__(self, Xq, Y, K, D, item_mask=None, ban_indptr=None,
                 ban_indices=None, item_cats=None, query_cats=None):
        Xq, Y = Xq.cpu().float(), Y.cpu().float()
        B, f = Xq.shape
        N = Y.shape[0]
        self.B, self.N, self.K, self.D = B, N, int(K), int(D)
        self.s = Xq.double() @ Y.double().t()
        self.sb = bf16_round(Xq) @ bf16_round(Y).t()
        self.tol = (f * 2.0 ** -23
                    * (Xq.double().abs() @ Y.double().abs().t()))
        cpu = [None if t is None else t.cpu() for t in
               (item_mask, ban_indptr, ban_indices, item_cats, query_cats)]
        self.valid = valid_items(B, N, *cpu)
        self.n_valid = self.valid.sum(dim=1)
        self.in_fp32_top = _separated_above(self.s, self.tol, self.valid,
                                            self.K)
        # the bound of a bf16 score's fp32 accumulation is that of the
        # rounded operands, which the unrounded ones bound within 2^-7
        self.in_bf16_top = _separated_above(self.sb, self.tol * 1.01,
                                            self.valid, self.D)
        self.must = self.in_fp32_top & self.in_bf16_top

    def slots(self):
        """Per query, how many of the K slots a correct answer fills."""
        return self.n_valid.clamp_max(self.K)

    def excluded_share(self):
        """Share of the (query, rank <= K) slots the oracle makes no claim
        about, i.e. that are not must-have."""
        total = int(self.slots().sum())
        if total == 0:
            return 0.0
        return (total - int(self.must.sum())) / total

    def fp32_rank(self, b, j):
        """1-based rank of valid item j by float64 score of fp32 inputs."""
        return self._rank(self.s, b, j)

    def bf16_rank(self, b, j):
        return self._rank(self.sb, b, j)

    def _rank(self, score, b, j):
        assert self.valid[b, j]
        row = score[b].masked_fill(~self.valid[b], NEG_INF)
        return int((row > row[j]).sum()) + 1

    def check(self, gv, gi):
        """Assert everything the contract promises of (values, indices);
        returns excluded_share()."""
        gv, gi = gv.cpu(), gi.cpu()
        B, K = self.B, self.K
        assert gv.shape == (B, K) and gi.shape == (B, K)
        assert gv.dtype == torch.float32 and gi.dtype == torch.int64
        filled = gi >= 0
        # padding: exactly the slots past n_valid, and exactly -1 / -inf
        want_filled = (torch.arange(K).unsqueeze(0)
                       < self.slots().unsqueeze(1))
        assert torch.equal(filled, want_filled), \
            f"filled slots differ in queries " \
            f"{(filled != want_filled).any(dim=1).nonzero().flatten().tolist()}"
        assert (gi[~filled] == -1).all()
        assert (gv[~filled] == NEG_INF).all()
        assert torch.isfinite(gv[filled]).all()
        assert (gi[filled] < self.N).all()
        safe = gi.clamp_min(0)
        # valid, distinct, descending
        assert self.valid.gather(1, safe)[filled].all(), \
            "a filtered item was returned"
        got = torch.zeros((B, self.N), dtype=torch.int32)
        got.scatter_add_(1, safe, filled.to(torch.int32))
        assert int(got.max()) <= 1, "an item was returned twice"
        gvd = gv.double().masked_fill(~filled, NEG_INF)
        assert (gvd[:, 1:] <= gvd[:, :-1]).all(), "values not descending"
        # values are the fp32 dots of the returned items
        want = self.s.gather(1, safe)
        err = (gvd - want).abs()[filled]
        lim = (1e-5 + 1e-5 * want.abs())[filled]
        assert (err <= lim).all(), \
            f"max |value - dot| {float(err.max()):.3e}"
        # every must-have item is there
        missing = self.must & (got == 0)
        assert not missing.any(), \
            f"must-have (query, item) pairs missing: " \
            f"{missing.nonzero().tolist()[:8]}"
        # the last filled slot is no worse than the contract allows: the
        # candidates hold every item of in_bf16_top, so the r-th returned
        # value is at least the r-th best fp32 dot among those (which is
        # at least the smallest must-have score whenever the must-have
        # set fills all r slots)
        r = self.slots()
        pool = self.s.masked_fill(~self.in_bf16_top, NEG_INF)
        pv, pi = torch.sort(pool, dim=1, descending=True)
        for b in range(B):
            rb = int(r[b])
            if rb == 0 or int(self.in_bf16_top[b].sum()) < rb:
                continue
            floor = float(pv[b, rb - 1])
            slack = (float(self.tol[b, pi[b, rb - 1]])
                     + 1e-5 + 1e-5 * abs(floor))
            assert float(gvd[b, rb - 1]) >= floor - slack, \
                f"query {b}: slot {rb} holds {float(gvd[b, rb - 1])}, " \
                f"the shortlist guarantees {floor}"
            mb = self.must[b]
            if int(mb.sum()) == rb:
                assert float(gvd[b, rb - 1]) >= float(self.s[b][mb].min()) \
                    - slack
        return self.excluded_share()


def check(gv, gi, Xq, Y, K, D, **filters):
    """One-shot form of Oracle(...).check(gv, gi)."""
    return Oracle(Xq, Y, K, D, **filters).check(gv, gi)


# ------------------------------------------------------------------ inputs

def designed_inversion(K, d, f, N, rows, B=1, qrow=0, seed=0):
    """An fp32/bf16 rank inversion exactly at the K cut, every number
    exact in fp32 and every bf16 product exact.

    Query row `qrow` is x = (1, 1, 0, ...). `rows` lists the K + d item
    rows that matter, in this order:
      K - 1 leaders  (2 + m, 2 + m, 0...), m = 1..K-1: score 4 + 2m;
      the target A   (1 + 3/1024, 1 + 3/1024): fp32 score 2 + 6/1024,
                     bf16 score 2 (bf16 keeps 8 bits: 1 + 3/1024 -> 1);
      d decoys       (1 + 5/1024, 1): fp32 score 2 + 5/1024, bf16 score
                     2 + 8/1024 (1 + 5/1024 -> 1 + 1/128).
    Every other item j is (-(j mod 7), 0, ...), score <= 0. So A has fp32
    rank K, ahead of the decoys by 2^-10, and bf16 rank K + d. (Rounding
    is monotone per coordinate; it takes two coordinates to invert.)
    The other query rows are small integers. Returns (Xq, Y, info)."""
    rows = [int(r) for r in rows]
    assert len(rows) == K + d and len(set(rows)) == K + d
    assert f >= 2 and max(rows) < N and 0 <= qrow < B
    g = torch.Generator().manual_seed(1000 + seed)
    Xq = torch.randint(-4, 5, (B, f), generator=g).float()
    Xq[qrow] = 0.0
    Xq[qrow, :2] = 1.0
    Y = torch.zeros((N, f))
    Y[:, 0] = -(torch.arange(N) % 7).float()
    leaders, a, decoys = rows[:K - 1], rows[K - 1], rows[K:]
    for m, r in enumerate(leaders, start=1):
        Y[r, :2] = 2.0 + m
    Y[a, :2] = 1.0 + 3.0 / 1024
    for r in decoys:
        Y[r, 0] = 1.0 + 5.0 / 1024
        Y[r, 1] = 1.0
    # best first: leader K-1 scores highest
    info = dict(qrow=qrow, target=a, leaders=leaders[::-1], decoys=decoys,
                fp32_top=leaders[::-1] + [a])
    return Xq, Y, info


def place_tail(N, K, d):
    """The K + d special rows are the last rows of the catalog, the
    target on row N - 1. Returns (N, rows) in designed_inversion's
    order."""
    n = K + d
    assert n <= N
    rest = list(range(N - n, N - 1))
    return N, rest[:K - 1] + [N - 1] + rest[K - 1:]


def place_per_chunk(K, d):
    """One special row in each 64-item chunk, at varying offsets, the
    last chunk partial (47 rows). Returns (N, rows)."""
    n = K + d
    N = 64 * n - 17
    return N, [64 * c + (7 * c + 3) % 47 for c in range(n)]


def clustered_catalog(B, N, f, seed):
    """Items scattered tightly (sigma 0.05) round one base row: scores of
    a query differ by far less than their size, so bf16 rounding of the
    items reorders them near every cut."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn((1, f), generator=g)
    Y = base + 0.05 * torch.randn((N, f), generator=g)
    Xq = torch.randn((B, f), generator=g)
    return Xq.float(), Y.float()


def int_problem(B, N, f, seed=0):
    """Small integers whose scores are DISTINCT within every query, exact
    in bf16 and in fp32 under any summation order, so every route must
    return the float64 reference bit for bit.

    Coordinates 0..f-3: x in 128 * {-1, 0, 1}, y in {-4, -2, 0, 2, 4}, so
    their part of a score is a multiple of 256 (|.| <= 512 (f - 2) <
    2^24). The last two carry the item's row number j < 256 as
    (j mod 16) * x + (j div 16) * 16 x with x = +-1 per query: two items
    of one query differ by a non-zero amount below 256 or by a multiple
    of 256 plus such an amount."""
    assert f >= 3 and N <= 256
    g = torch.Generator().manual_seed(500 + 7 * N + f + seed)
    Xq = torch.zeros((B, f))
    Y = torch.zeros((N, f))
    Xq[:, :f - 2] = 128.0 * torch.randint(-1, 2, (B, f - 2), generator=g)
    Y[:, :f - 2] = 2.0 * torch.randint(-2, 3, (N, f - 2), generator=g)
    sign = 1.0 - 2.0 * torch.randint(0, 2, (B,), generator=g)
    Xq[:, f - 2] = sign
    Xq[:, f - 1] = 16.0 * sign
    j = torch.arange(N)
    Y[:, f - 2] = (j % 16).float()
    Y[:, f - 1] = (j // 16).float()
    return Xq, Y


def reference_topk(Xq, Y, K, valid=None):
    """Float64 top-K with the package's padding convention: (values
    float32 [B, K], indices int64 [B, K]), empty slots -inf / -1. Meant
    for inputs whose float64 scores are fp32-exact and distinct."""
    s = Xq.double() @ Y.double().t()
    if valid is not None:
        s = s.masked_fill(~valid, NEG_INF)
    B, N = s.shape
    kc = min(K, N)
    v, i = torch.topk(s, kc, dim=1)
    i = i.masked_fill(v == NEG_INF, -1)
    if kc < K:
        v = torch.cat([v, torch.full((B, K - kc), NEG_INF,
                                     dtype=v.dtype)], 1)
        i = torch.cat([i, torch.full((B, K - kc), -1, dtype=i.dtype)], 1)
    return v.float(), i
