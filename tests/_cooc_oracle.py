"""Shared fixtures of the co-occurrence tests: a brute-force pair
counter in plain Python and the data sets both test files use."""

from collections import defaultdict

import torch

# (U, N, nnz, n): the shapes on which the template's lexsort order and
# the packed-key order were checked to agree
SHAPES = [(300, 200, 2500, 10), (50, 30, 600, 64), (400, 1000, 3000, 1)]


def random_pairs(n_users, n_items, nnz, seed):
    """nnz random (user, item) pairs with duplicates among them; the
    last item is viewed by nobody and the last user views one item."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, n_users - 1, (nnz - 1,), generator=g)
    i = torch.randint(0, n_items - 1, (nnz - 1,), generator=g)
    return (torch.cat([u, torch.tensor([n_users - 1])]),
            torch.cat([i, torch.tensor([0])]))


def brute_force(users, items, n):
    """item -> [(other, count)] for the items that have a neighbour:
    count descending, id ascending, at most n."""
    views = defaultdict(set)
    for u, i in zip(users.tolist(), items.tolist()):
        views[u].add(i)
    counts = defaultdict(lambda: defaultdict(int))
    for its in views.values():
        for a in its:
            for b in its:
                if a != b:
                    counts[a][b] += 1
    return {a: sorted(row.items(), key=lambda jc: (-jc[1], jc[0]))[:n]
            for a, row in counts.items()}


def arrays_to_dict(top_ids, top_cnt):
    """The [N, n] arrays as the brute-force dict; checks the padding."""
    ids, cnt = top_ids.cpu(), top_cnt.cpu()
    assert ids.dtype == torch.int32 and cnt.dtype == torch.int32
    assert torch.equal(ids < 0, cnt == 0)
    assert bool(((ids == -1) | (ids >= 0)).all())
    out = {}
    for it in range(ids.shape[0]):
        k = int((ids[it] >= 0).sum())
        assert bool((ids[it, k:] == -1).all())  # padding only at the end
        if k:
            out[it] = list(zip(ids[it, :k].tolist(), cnt[it, :k].tolist()))
    return out


def star(n_users, per_user, extra):
    """Item 0 viewed by n_users users who each view per_user items of
    their own besides, and by `extra` users who each view one more item
    of their own: item 0 has exactly n_users * per_user + extra distinct
    neighbours and a routing bound equal to that number."""
    u, i = [], []
    nxt = 1
    for k in range(n_users + extra):
        m = per_user if k < n_users else 1
        u += [k] * (m + 1)
        i += [0] + list(range(nxt, nxt + m))
        nxt += m
    return (torch.tensor(u), torch.tensor(i), n_users + extra, nxt)


def rising(n_uniq_users, n_win):
    """Item 0 with n_uniq_users * 64 + n_win distinct neighbours. Its
    first users each bring 64 count-1 items of their own; its LAST users
    view nested subsets of n_win winner items (user t of them views
    winners 2t, 2t + 1, ...), so winner k has count k // 2 + 1: the
    counts seen rise along the user list and the top of the row sits at
    its end, with ties in pairs."""
    u, i = [], []
    nxt = 1
    for k in range(n_uniq_users):
        u += [k] * 65
        i += [0] + list(range(nxt, nxt + 64))
        nxt += 64
    win = list(range(nxt, nxt + n_win))
    k = n_uniq_users
    for t in range(0, n_win, 2):
        u += [k] * (1 + n_win - t)
        i += [0] + win[t:]
        k += 1
    return torch.tensor(u), torch.tensor(i), k, nxt + n_win
