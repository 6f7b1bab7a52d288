"""Numpy restatement of `Preprocessor.process` (daisy/utils/loader.py:176-189) and of every split of
daisy/utils/splitter.py, stage by stage as DESIGN.md §21 lists them, plus the FIXTURES the golden file and the GPU tests
share.  Fixtures are rebuilt from their seeds; tests/golden/make_golden_prep.py asserts that this oracle equals the real
reference on every fixture the reference can serve before it writes tests/golden/kat_prep.npz.

  dedup      stable argsort of the (user, item) pair key; the tail of a run is the largest row number (keep='last')
  threshold  rating >= t, NaN dropped
  filter     one bincount of the frame as it stands, one mask
  ui core    repeated bincount rounds: a row dies when its user's or its item's live count is < N; the counts are taken
             at the start of the round.  `rounds` counts the rounds that removed rows.
  encoding   np.unique(return_inverse) of the survivors
  time sort  stable argsort (the reference's quicksort leaves ties open: fixtures with `ties` are oracle-only)
  item_pop   bincount / user_num, one fp64 division

Random splits: the key of row r in fold f is Philox4x32-10 with counter (r, SPLIT_STREAM | f) and key seed - the
library's generator (oracle/bpr_mf_numpy.py::_draw_u64 is the scalar form; `philox_u64` below is the same function on
arrays, checked against it in test_oracle_prep.py).
"""
import re

import numpy as np

SPLIT_STREAM = 1 << 59
_M32 = np.uint64(0xFFFFFFFF)


# ---- Preprocessor ------------------------------------------------------------------------------------------------------
def codes_dtype(k):
    for dt in (np.int8, np.int16, np.int32):
        if k < np.iinfo(dt).max:          # pandas' coerce_indexer_dtype: 127 categories are already int16
            return np.dtype(dt)
    return np.dtype(np.int64)


def dedup_last(user, item):
    cu = np.unique(user, return_inverse=True)[1].astype(np.int64)
    ci = np.unique(item, return_inverse=True)[1].astype(np.int64)
    key = cu * (int(ci.max()) + 1 if len(ci) else 1) + ci
    order = np.argsort(key, kind="stable")
    ks = key[order]
    tail = np.ones(len(ks), dtype=bool)
    tail[:-1] = ks[1:] != ks[:-1]
    keep = np.zeros(len(ks), dtype=bool)
    keep[order[tail]] = True
    return keep


def core_filter(cu, ci, keep, prepro, level):
    """cu / ci: dense codes of all rows; keep: the live mask.  -> (mask, rounds)"""
    if prepro == "origin":
        return keep, 0
    N = int(re.findall(r"\d+", prepro)[0])
    nu, ni = int(cu.max()) + 1, int(ci.max()) + 1
    keep = keep.copy()
    peel = prepro.endswith("core") and level == "ui"
    rounds = 0
    while True:
        ucnt, icnt = np.bincount(cu[keep], minlength=nu), np.bincount(ci[keep], minlength=ni)
        bad = np.zeros(len(cu), dtype=bool)
        if "u" in level:
            bad |= ucnt[cu] < N
        if "i" in level:
            bad |= icnt[ci] < N
        bad &= keep
        if not peel:
            return keep & ~bad, 0
        if not bad.any():
            return keep, rounds
        keep &= ~bad
        rounds += 1


def process(user, item, rating, ts, prepro="origin", level="ui", threshold=None, want_pop=True):
    user, item, ts = np.asarray(user), np.asarray(item), np.asarray(ts)
    n = len(user)
    keep = dedup_last(user, item) if n else np.zeros(0, dtype=bool)
    if threshold is not None:
        with np.errstate(invalid="ignore"):
            keep &= np.asarray(rating, dtype=np.float64) >= threshold
    if n:
        cu = np.unique(user, return_inverse=True)[1]
        ci = np.unique(item, return_inverse=True)[1]
        keep, rounds = core_filter(cu, ci, keep, prepro, level)
    else:
        rounds = 0
    rows = np.flatnonzero(keep)
    utok, ucode = np.unique(user[rows], return_inverse=True)
    itok, icode = np.unique(item[rows], return_inverse=True)
    order = np.argsort(ts[rows].astype("int64") if ts.dtype.kind == "M" else ts[rows], kind="stable")
    rows, ucode, icode = rows[order], ucode[order], icode[order]
    user_num, item_num = len(utok), len(itok)
    with np.errstate(invalid="ignore", divide="ignore"):
        pop = np.bincount(icode, minlength=item_num) / user_num if want_pop else None
    return {"rows": rows.astype(np.int64), "user": ucode.astype(codes_dtype(user_num)),
            "item": icode.astype(codes_dtype(item_num)), "uid_token": utok, "iid_token": itok, "item_pop": pop,
            "user_num": user_num, "item_num": item_num, "rounds": rounds}


# ---- splits ------------------------------------------------------------------------------------------------------------
def philox_u64(seed, stream, idx):
    idx = np.asarray(idx, dtype=np.uint64)
    c0, c1 = idx & _M32, idx >> np.uint64(32)
    c2 = np.full_like(idx, np.uint64(stream & 0xFFFFFFFF))
    c3 = np.full_like(idx, np.uint64((stream >> 32) & 0xFFFFFFFF))
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1),
                          p0 & _M32)
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return (c1 << np.uint64(32)) | c0


def _groups(user, order):
    """the rows `order` regrouped by user (stable) -> (grouped rows, position inside the group, group length per row)"""
    code = np.unique(user, return_inverse=True)[1]
    g = order[np.argsort(code[order], kind="stable")]
    cg = code[g]
    cnt = np.bincount(code)
    start = np.cumsum(cnt) - cnt
    return g, np.arange(len(g)) - start[cg], cnt[cg]


def _finish(n, test):
    return np.setdiff1d(np.arange(n, dtype=np.int64), test), test.astype(np.int64)


def split_tloo(user, ts):
    user, ts = np.asarray(user), np.asarray(ts)
    ts = ts.astype("int64") if ts.dtype.kind == "M" else ts
    n = len(user)
    # per user: the largest timestamp, ties to the earliest row
    code = np.unique(user, return_inverse=True)[1]
    order = np.lexsort((np.arange(n), _desc_key(ts), code))
    code = code[order]
    head = np.ones(n, dtype=bool)
    head[1:] = code[1:] != code[:-1]
    return _finish(n, np.sort(order[head]))


def _desc_key(ts):
    """an integer key that sorts timestamps descending without overflow: the rank of -ts"""
    return -np.unique(ts, return_inverse=True)[1]


def utfo_split_len(length, size):
    return int(np.ceil(length * (1 - size)))                    # splitter.py:61


def ufo_head(length, size):
    return int(round(length * size))                            # DataFrame.sample(frac=size)


def split_utfo(user, size):
    n = len(user)
    g, pos, ln = _groups(np.asarray(user), np.arange(n))
    cut = np.array([utfo_split_len(int(l), size) for l in range(int(ln.max()) + 1)])[ln] if n else ln
    return _finish(n, g[pos >= cut])


def split_random(method, n, user=None, size=0.5, seed=2022, fold=0):
    key = philox_u64(seed, SPLIT_STREAM | fold, np.arange(n))
    order = np.argsort(key, kind="stable")
    if method == "rsbr":
        return _finish(n, order[:int(n * size)])
    g, pos, ln = _groups(np.asarray(user), order)
    if method == "rloo":
        return _finish(n, g[pos == 0])
    head = np.array([ufo_head(int(l), size) for l in range(int(ln.max()) + 1)])[ln]
    return _finish(n, g[pos < head])


def split_tsbr(n, size):
    k = int(np.ceil(n * (1 - size)))
    return np.arange(k), np.arange(k, n)


def split_cv(n, k):
    sizes = np.full(k, n // k)
    sizes[:n % k] += 1
    stop = np.cumsum(sizes)
    ids = np.arange(n)
    return [(np.concatenate([ids[:a], ids[b:]]), ids[a:b]) for a, b in zip(stop - sizes, stop)]


# ---- fixtures ----------------------------------------------------------------------------------------------------------
def _ids(codes, kind, prefix):
    codes = np.asarray(codes, dtype=np.int64)
    if kind == "dense":
        return codes
    if kind == "sparse":
        return codes * 7919 + 13
    if kind == "neg":
        return codes * 3 - 100
    if kind == "big":
        return codes * 5 + (1 << 33)
    if kind == "str":
        return np.array([f"{prefix}{c:05d}" for c in codes], dtype=object)
    raise ValueError(kind)


def _chain(length):
    """a path u0-i0-u1-i1-...: `length` edges; the 2-core peels it from both ends, one edge per end and round"""
    e = np.arange(length)
    return (e + 1) // 2, e // 2


# tag -> how the frame is built; prepro / level / threshold: the Preprocessor's config.  `ties`: heavy timestamp ties -
# the reference's unstable sort cannot serve, the GPU test compares against the oracle alone (not in the golden file).
PREP_FIXTURES = {}
for _n in (1, 255, 256, 257, 1000):
    PREP_FIXTURES[f"n{_n}"] = dict(kind="rand", n=_n, U=max(_n // 12, 1), I=max(_n // 9, 1), prepro="origin", level="ui", seed=_n)
for _p in ("origin", "3filter", "3core"):
    for _l in ("ui", "u", "i"):
        PREP_FIXTURES[f"{_p}_{_l}"] = dict(kind="rand", n=1000, U=90, I=120, prepro=_p, level=_l, seed=7)
PREP_FIXTURES.update({
    "sparse": dict(kind="rand", n=600, U=40, I=50, ids="sparse", prepro="2core", level="ui", seed=11),
    "neg": dict(kind="rand", n=600, U=40, I=50, ids="neg", prepro="2filter", level="ui", seed=12),
    "big": dict(kind="rand", n=600, U=40, I=50, ids="big", prepro="3core", level="ui", seed=13),
    "str": dict(kind="rand", n=600, U=40, I=50, ids="str", prepro="3core", level="ui", seed=14),
    "triple": dict(kind="triple", n=300, U=20, I=25, prepro="origin", level="ui", seed=15, threshold=3.0),
    "onepair": dict(kind="onepair", n=500, prepro="origin", level="ui", seed=16),
    "thresh": dict(kind="rand", n=700, U=50, I=60, prepro="2core", level="ui", seed=17, threshold=3.0, nan=True),
    "stairs": dict(kind="stairs", chain=24, prepro="2core", level="ui", seed=18),
    "empty": dict(kind="empty", n=300, prepro="5core", level="ui", seed=19),
    "hotitem": dict(kind="hot", n=2000, U=300, I=200, hot="item", prepro="3core", level="ui", seed=20),
    "hotuser": dict(kind="hot", n=2000, U=300, I=200, hot="user", prepro="3core", level="ui", seed=21),
    "users126": dict(kind="count", users=126, prepro="origin", level="ui", seed=28),
    "users127": dict(kind="count", users=127, prepro="origin", level="ui", seed=22),
    "users128": dict(kind="count", users=128, prepro="origin", level="ui", seed=23),
    "users129": dict(kind="count", users=129, prepro="origin", level="ui", seed=24),
    # either side of the size at which the id sorts change algorithm (kIdSortMergeLimit), heavy ties: stability in both
    "ties_below": dict(kind="rand", n=262143, U=4000, I=3000, prepro="5core", level="ui", seed=25, ties=True),
    "ties_above": dict(kind="rand", n=262145, U=4000, I=3000, prepro="5core", level="ui", seed=26, ties=True),
    "ties_small": dict(kind="rand", n=1000, U=90, I=120, prepro="3core", level="ui", seed=27, ties=True),
})


def prep_frame(fx):
    """-> dict of columns user, item, rating (float64), timestamp (int64): the raw frame of a fixture"""
    rng = np.random.default_rng(fx["seed"])
    kind = fx["kind"]
    if kind == "rand":
        n = fx["n"]
        u, i = rng.integers(0, fx["U"], n), rng.integers(0, fx["I"], n)
    elif kind == "triple":
        n = fx["n"]
        u, i = rng.integers(0, fx["U"], n), rng.integers(0, fx["I"], n)
        u[[5, 120, 290]], i[[5, 120, 290]] = 3, 4
    elif kind == "onepair":
        n = fx["n"]
        u, i = np.full(n, 7), np.full(n, 9)
    elif kind == "stairs":
        cu, ci = _chain(fx["chain"])
        bu, bi = np.meshgrid(np.arange(3) + 100, np.arange(3) + 100)            # a 3 x 3 block that survives
        u, i = np.concatenate([cu, bu.ravel()]), np.concatenate([ci, bi.ravel()])
        p = rng.permutation(len(u))
        u, i, n = u[p], i[p], len(u)
    elif kind == "empty":
        n = fx["n"]
        u, i = np.arange(n), rng.integers(0, 40, n)
    elif kind == "hot":
        n = fx["n"]
        u, i = rng.integers(0, fx["U"], n), rng.integers(0, fx["I"], n)
        half = rng.permutation(n)[:n // 2]
        if fx["hot"] == "item":
            i[half] = 3
            u[half] = rng.permutation(n)[:n // 2] % fx["U"]
        else:
            u[half] = 3
    elif kind == "count":
        n = fx["users"] * 2
        u, i = np.repeat(rng.permutation(fx["users"]), 2), rng.permutation(n)
    else:
        raise ValueError(kind)
    rating = rng.integers(1, 6, n).astype(np.float64)
    if kind == "triple":
        rating[[5, 120, 290]] = (5.0, 5.0, 3.0)         # the last copy is the one that stays, at the threshold
    if fx.get("nan"):
        rating[rng.permutation(n)[:n // 20]] = np.nan
    ts = rng.integers(0, 16, n) if fx.get("ties") else rng.permutation(n) * 3 - n
    ids = fx.get("ids", "dense")
    return {"user": _ids(u, ids, "u"), "item": _ids(i, ids, "i"), "rating": rating, "timestamp": ts.astype(np.int64)}


UTFO_SIZES = (0.1, 0.2, 0.3, 0.5, 0.9)
SPLIT_FIXTURES = {
    # users of 1, 2 and 64 rows and every length 1 .. 40, blocks in shuffled user order (user-contiguous)
    "blocks": dict(lengths=[1, 2, 64] + list(range(1, 41)), contiguous=True, seed=31),
    # the same users with their rows interleaved: the reference's utfo cannot serve
    "mixed": dict(lengths=[1, 2, 64] + list(range(1, 41)), contiguous=False, seed=32),
    # products 0.5, 1.5, 2.5 at size 0.1 round to 0, 2, 2: the first user contributes nothing
    "ufo_round": dict(lengths=[5, 15, 25, 10, 30], contiguous=True, seed=33),
}
CV_CASES = ((10, 3), (11, 4), (257, 5), (8, 8))
TSBR_CASES = ((10, 0.2), (257, 0.1), (1000, 0.3), (7, 0.5))


def split_frame(fx):
    """-> user (sparse int64 ids), timestamp int64.  Timestamps tie inside a user: the maximum of every user with three
    rows or more is held by three of its rows."""
    rng = np.random.default_rng(fx["seed"])
    lengths = np.asarray(fx["lengths"])
    uid = rng.permutation(len(lengths)) * 11 + 5
    user = np.repeat(uid, lengths)
    if not fx["contiguous"]:
        user = user[rng.permutation(len(user))]
    n = len(user)
    ts = rng.integers(0, 1000, n).astype(np.int64)
    for u in np.unique(user):
        r = np.flatnonzero(user == u)
        if len(r) >= 3:
            ts[rng.permutation(r)[:3]] = 5000
    return user.astype(np.int64), ts
