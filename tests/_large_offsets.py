"""Planted rows for the large-offset tests (CPU-only code; the GPU tests
import it too).

A factor matrix of N = 2^24 + 64 rows is described by its few non-zero
rows, so that nothing here allocates it. With rowbytes = F * element
size, row r starts at byte r * rowbytes and element r * F:

    band A  rows below the 2 GiB byte offset
    band B  rows in [2 GiB, 4 GiB)
    band C  rows at or past 4 GiB
    band D  rows at or past element 2^31 (fp32 F = 128: row 2^24;
            bf16 F = 128: the same row as the 4 GiB threshold)

Planted are the last row of each band and the first of the next, N - 1,
and alias groups a, a + 2 GiB / rowbytes, a + 4 GiB / rowbytes (and
a + 2^31 / F) for a in ALIAS_BASE. Planted row number i (ascending row
order) holds two small integers,

    y[(3 i) % (F - 1)] = sign_i v_i        y[F - 1] = sign_i

with the v_i a permutation of 1 .. P and sign_i = -1 for i % 6 == 5, so
against the query m * ones its score is m sign_i (v_i + 1): distinct,
exact in bf16 and fp32, and not monotone in the row number. Every other
row is zero and scores 0.

`resolve` maps a row to the row a kernel would fetch if it carried the
byte offset or the element index of the row start in 32 bits. A fetch
below the buffer (a negative signed offset) is a fault: None. The
operations below are written against `resolve`, so the same code gives
the expected result (model "exact") and what a narrowed kernel would
give; tests/test_large_offsets_cpu.py asserts that these differ.
"""

import math

import torch

GIB = 1 << 30
N_ROWS = 2 ** 24 + 64
ALIAS_BASE = (3, 17, 40)

MODELS = ("byte_i32", "byte_u32", "elem_i32")


class Tier:
    def __init__(self, name, f, esize, n=N_ROWS):
        self.name, self.f, self.esize, self.n = name, f, esize, n
        self.rowbytes = f * esize
        self.r2 = 2 * GIB // self.rowbytes      # first row of band B
        self.r4 = 4 * GIB // self.rowbytes      # first row of band C
        self.rd = 2 ** 31 // f                  # first row of band D
        self.nbytes = n * self.rowbytes

    def thresholds(self):
        """First rows of the bands B, C and D that the matrix reaches."""
        return sorted({t for t in (self.r2, self.r4, self.rd) if t < self.n})

    def band(self, row):
        if row >= self.rd:
            return "D"
        return "A" if row < self.r2 else "B" if row < self.r4 else "C"

    def __repr__(self):
        return self.name


TIERS = {t.name: t for t in (
    Tier("fp32_f64", 64, 4),     # 4 GiB tier
    Tier("fp32_f128", 128, 4),   # 8 GiB tier
    Tier("bf16_f128", 128, 2),   # 4 GiB = 2^31 elements
    Tier("bf16_f64", 64, 2),     # the bf16 copy of fp32_f64: 2 GiB
)}


def planted_rows(tier):
    rows = {tier.n - 1}
    for t in tier.thresholds():
        rows |= {t - 1, t}
    for a in ALIAS_BASE:
        rows |= {a} | {a + t for t in tier.thresholds() if a + t < tier.n}
    return sorted(rows)


class Planted:
    """rows (ascending), vec[row] (float64 [F]) and score1[row], the
    score against the all-ones query."""

    def __init__(self, tier):
        self.tier = tier
        self.rows = planted_rows(tier)
        P, f = len(self.rows), tier.f
        mult = next(m for m in (5, 7, 11, 13) if math.gcd(m, P) == 1)
        self.vec, self.score1 = {}, {}
        for i, r in enumerate(self.rows):
            sign = -1 if i % 6 == 5 else 1
            v = 1 + (i * mult) % P
            y = torch.zeros(f, dtype=torch.float64)
            y[(3 * i) % (f - 1)] = sign * v
            y[f - 1] = sign
            self.vec[r] = y
            self.score1[r] = sign * (v + 1)
        assert len(set(self.score1.values())) == P

    def dense_rows(self, dtype=torch.float32):
        """(row ids int64 [P], values [P, F]) to write into a zero matrix."""
        return (torch.tensor(self.rows),
                torch.stack([self.vec[r] for r in self.rows]).to(dtype))

    def positive(self):
        return [r for r in self.rows if self.score1[r] > 0]


# ------------------------------------------------------ addressing models

def _wrap(v, signed):
    v &= 0xFFFFFFFF
    return v - 2 ** 32 if signed and v >= 2 ** 31 else v


def resolve(tier, model, row):
    """The row fetched for `row` under `model`; None = outside the buffer."""
    if model == "exact":
        return row
    kind, width = model.split("_")
    unit = tier.rowbytes if kind == "byte" else tier.f
    off = _wrap(row * unit, width == "i32")
    if off < 0 or off // unit >= tier.n:
        return None
    return off // unit


def _period(tier, model):
    unit = tier.rowbytes if model.startswith("byte") else tier.f
    return 2 ** 32 // unit


def differs(tier, model):
    """Whether `model` fetches another row than asked for, for any row."""
    lo = 2 ** 31 // (tier.rowbytes if model.startswith("byte") else tier.f)
    return any(resolve(tier, model, r) != r
               for r in (lo, _period(tier, model)) if r < tier.n)


def _sources(tier, model, rows):
    """All j in [0, n) with resolve(j) in rows."""
    per = _period(tier, model) if model != "exact" else tier.n
    out = set()
    for r in rows:
        j = r % per
        while j < tier.n:
            if resolve(tier, model, j) == r:
                out.add(j)
            j += per
    return out


class View:
    """What a kernel sees of the planted matrix under one model."""

    def __init__(self, planted, model="exact"):
        self.p, self.tier, self.model = planted, planted.tier, model
        self.faulted = False

    def fetch(self, row):
        m = resolve(self.tier, self.model, row)
        if m is None:
            self.faulted = True     # counted, and read as zeros
        return self.p.vec.get(m) if m is not None else None

    def score(self, row, mult=1):
        y = self.fetch(row)
        return 0 if y is None else int(mult * y.sum())

    def scan(self, mult=1):
        """{row: score} of every row a full pass scores non-zero. A pass
        touches all rows, so any row outside the buffer is a fault."""
        t = self.tier
        if self.model.endswith("i32"):
            unit = t.rowbytes if self.model.startswith("byte") else t.f
            if 2 ** 31 // unit < t.n:
                self.faulted = True
        out = {}
        for j in _sources(t, self.model, self.p.rows):
            s = self.score(j, mult)
            if s != 0:
                out[j] = s
        return out


# --------------------------------------------------------------- operations
# Each returns plain Python data, equal iff the outputs are equal.

def op_topk(view, K, mults=(1,), banned=()):
    """Per query (score, id) of the K best, score descending."""
    res = []
    for m in mults:
        sc = [(s, j) for j, s in view.scan(m).items()
              if s > 0 and j not in banned]
        sc.sort(key=lambda e: (-e[0], e[1]))
        # the zero rows never reach the expected list
        assert view.model != "exact" or len(sc) >= K
        res.append(sc[:K])
    return res


def op_slice_lists(view, n_slices, interleave, chunk=64):
    """{slice: sorted (id, score)} of the rows scoring > 0, as the raw
    per-slice lists of the MFMA kernel hold them."""
    n = view.tier.n
    per = -(-n // n_slices)
    out = {}
    for j, s in view.scan().items():
        if s > 0:
            sl = (j // chunk) % n_slices if interleave else j // per
            out.setdefault(sl, []).append((j, s))
    return {k: sorted(v) for k, v in out.items()}


def op_gather_dots(view, ids, mult=1):
    """x . Y[id] for listed ids: rescore, candidate lists, loss, targets."""
    return [view.score(j, mult) for j in ids]


def op_rank_counts(view, targets, seen, mult=1):
    """(gt, eq) per target against all rows but `seen` (and the target)."""
    n = view.tier.n
    nz = view.scan(mult)
    seen = set(seen)
    zeros = n - len(nz) - len([j for j in seen if j not in nz])
    res = []
    for t in targets:
        ts = view.score(t, mult)
        gt = sum(s > ts for j, s in nz.items() if j not in seen)
        eq = sum(s == ts for j, s in nz.items() if j not in seen and j != t)
        gt += zeros if 0 > ts else 0
        eq += (zeros - (1 if t not in nz and t not in seen else 0)) \
            if ts == 0 else 0
        res.append((gt, eq))
    return res


def op_loss(view, x_rows, indptr, indices, values):
    """(A, B, pred) of the explicit residual sums; x_rows[u] multiplies
    the all-ones query of CSR row u."""
    A = B = 0
    pred = []
    for u in range(len(indptr) - 1):
        for p in range(indptr[u], indptr[u + 1]):
            s = view.score(indices[p], x_rows[u])
            pred.append(s)
            A += (values[p] - s) ** 2
            B += s * s
    return A, B, pred


def xform_matrix(f):
    """A small-integer [F, F] matrix with y W != y for every planted y."""
    k = torch.arange(f)
    return (((3 * k[:, None] + 5 * k[None, :]) % 7) - 3).double()


def op_xform(view, W):
    """Non-zero rows after the in-place row transform: row j is read and
    written where the model puts it."""
    out = {r: tuple(v.tolist()) for r, v in view.p.vec.items()}
    for j in sorted(_sources(view.tier, view.model, view.p.rows)):
        m = resolve(view.tier, view.model, j)
        if m is not None:
            out[m] = tuple((view.p.vec[m] @ W).tolist())
    view.scan()  # a full pass: flags the fault of a signed model
    return out


def op_gathered(view, lists):
    """The rows a solver gathers for each CSR row; its arithmetic is a
    function of these alone."""
    out = []
    for cols in lists:
        got = []
        for c in cols:
            y = view.fetch(c)
            got.append(None if y is None else tuple(y.tolist()))
        out.append(got)
    return out


def op_output_rows(view, rows):
    """Where the result rows land in a NaN-filled output: {row: tag},
    every other row left unwritten."""
    out = {}
    for i, r in enumerate(rows):
        m = resolve(view.tier, view.model, r)
        if m is None:
            view.faulted = True
        else:
            out[m] = i
    return out
