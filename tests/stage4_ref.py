"""Stage 4 (stable per-activation bucketing): a numpy reference, a Python restatement of the launcher's plan functions,
seeded batch builders, and the width matrix that tests/test_gpu_stage4_widths.py runs (no GPU needed here).

bucket_ref is the expected output of every stage-4 comparison: a stable argsort of min(act, n_act) and the prefix of the
per-key counts (ActivationData.EnqueueMessage FIFO, ActivationData.cs:483-514; the oracle's ref_bucket keeps one vector
per bucket, too slow and too large at 2^26 buckets).  plan_of / route_items / msd_items restate make_plan,
make_bucket_plan (default ORL_LB_CEIL), route_items and msd_items of orl_internal.h / route_kernels.hip with the
constants read from those sources; the GPU tests use them to choose inputs and to assert what the matrix covers, never as
an expected output.  tests/test_stage4_ref.py pins all of it.
"""
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NO_ACT = 0xFFFFFFFF  # ORL_NO_ACT


# ---- the reference ------------------------------------------------------------------------------------------
def bucket_ref(act, n_act):
    """(order[n], offsets[n_act + 2]) as uint32: messages grouped by key = min(act, n_act) in arrival order, and where
    each key's group starts (offsets[n_act + 1] = n)."""
    key = np.minimum(np.ascontiguousarray(act, np.uint32), np.uint32(n_act))
    order = order_ref(act, n_act)
    if n_act + 1 <= 8 * len(key):
        offsets = np.zeros(n_act + 2, np.uint32)
        np.cumsum(np.bincount(key, minlength=n_act + 1), out=offsets[1:], dtype=np.uint32)
        return order, offsets
    # far more buckets than messages (2^27 buckets: the counts and their prefix are two gigabyte-sized passes)
    return order, np.repeat(*offsets_runs(act, n_act))


def order_ref(act, n_act):
    """bucket_ref's order alone."""
    key = np.minimum(np.ascontiguousarray(act, np.uint32), np.uint32(n_act))
    return np.argsort(key, kind="stable").astype(np.uint32)


def offsets_runs(act, n_act):
    """bucket_ref's offsets in run-length form, (totals uint32, runs int64) with np.repeat(totals, runs) == offsets: 0 up
    to and including the first key present, then each present key's running total up to and including the next one, n
    after the last.  The GPU tests of the LSD widths expand it on the device instead of moving 512 MB per batch."""
    key = np.minimum(np.ascontiguousarray(act, np.uint32), np.uint32(n_act))
    uk, cnt = np.unique(key, return_counts=True)
    totals = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    runs = np.diff(np.concatenate([[0], uk.astype(np.int64) + 1, [n_act + 2]]))
    return totals, runs


# ---- the plan, restated ---------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(ROOT, "orleans_amd", "csrc", name)) as f:
        return f.read()


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    v = m.group(1)
    if "<<" in v:  # "8u << 20"
        a, b = (int(x.strip().rstrip("u")) for x in v.split("<<"))
        return a << b
    return int(v.rstrip("u"))


_H = _src("orl_internal.h")
_K = _src("route_kernels.hip")
K_MAX_DIGIT_BITS = _const(_H, r"constexpr uint32_t kMaxDigitBits = (\d+);")
K_ROUTE_THREADS = _const(_H, r"constexpr uint32_t kRouteThreads = (\d+);")
K_ITEMS = _const(_H, r"constexpr uint32_t kItems = (\d+);")
K_MAX_ROUTE_ROWS = _const(_H, r"constexpr uint32_t kMaxRouteRows = (\d+);")
K_MSD_ITEMS = _const(_K, r"constexpr uint32_t kMsdItems = (\d+);")
K_MSD_ITEMS_SMALL = _const(_K, r"constexpr uint32_t kMsdItemsSmall = (\d+);")
K_MSD_SMALL_MAX = _const(_K, r"constexpr uint32_t kMsdSmallMax = ([0-9u]+ << \d+);")
K_ROUTE_MIN_WG = _const(_K, r"uint32_t route_min_wgs\(\) \{[^}]*?return x > 0 \? \(uint32_t\)x : (\d+)u;")
K_HOT_MIN_BATCH = _const(_K, r"constexpr uint32_t kHotMinBatch = ([0-9u]+ << \d+),")
K_HOT_SHARE = _const(_K, r"kHotShare = (\d+),")
_m = re.search(r"kHotMinCount = (\d+) \* (\d+);", _K)
K_HOT_MIN_COUNT = int(_m.group(1)) * int(_m.group(2))

# lsd: the LSD passes' digit widths, low digit first (empty on the two-level plan); hb == 0: one level
Plan = namedtuple("Plan", "w two_level hb lb lsd max_items")


def bit_length(n_act):
    return max(int(n_act).bit_length(), 1)


def make_plan(max_key):
    """make_plan: passes of <= kMaxDigitBits bits, low digit first, the extra bits to the low digits."""
    total = bit_length(max_key)
    passes = (total + K_MAX_DIGIT_BITS - 1) // K_MAX_DIGIT_BITS
    base, extra = divmod(total, passes)
    return tuple(base + (1 if i < extra else 0) for i in range(passes))


def plan_of(n_act):
    """make_bucket_plan(n_act) (keys in [0, n_act]) and max_route_items(n_act)."""
    w = bit_length(n_act)
    two = w <= 2 * K_MAX_DIGIT_BITS
    lb = w if w <= K_MAX_DIGIT_BITS else w // 2
    hb = w - lb
    return Plan(w, two, hb if two else 0, lb if two else 0, () if two else make_plan(n_act),
                K_MSD_ITEMS if two and hb > 0 else K_ITEMS)


def _ceil_div(a, b):
    return -(-a // b)


def route_items(n, max_items=K_ITEMS, min_wg=K_ROUTE_MIN_WG):
    """route_items: messages per thread of the route kernel (= the rows of pass 0's histogram)."""
    items = max_items
    while (items > 1 and _ceil_div(n, K_ROUTE_THREADS * items) < min_wg
           and _ceil_div(n, K_ROUTE_THREADS * (items >> 1)) <= K_MAX_ROUTE_ROWS):
        items >>= 1
    return items


def msd_items(n, items):
    return K_MSD_ITEMS_SMALL if n <= K_MSD_SMALL_MAX and items <= K_MSD_ITEMS_SMALL else K_MSD_ITEMS


def row_step0(n_act, n, items=None):
    """Which of pass 0's histogram rows the reading pass uses (every row_step0-th); None: no histogram (one level).
    items: the producer's messages per thread (default: the route kernel's; orl_bucket_device always has kItems)."""
    p = plan_of(n_act)
    items = route_items(n, p.max_items) if items is None else items
    if p.two_level:
        return msd_items(n, items) // items if p.hb > 0 else None
    return K_ITEMS // items


def route_item_ranges(max_items=K_ITEMS, min_wg=K_ROUTE_MIN_WG):
    """{items: (first n, last n or None)} by bisection over route_items (monotone in n)."""
    out, lo = {}, 1
    it = 1
    while it <= max_items:
        if it == max_items:
            out[it] = (lo, None)
            break
        a, b = lo, 1 << 40  # route_items(a) <= it < route_items(b)
        while b - a > 1:
            m = (a + b) // 2
            if route_items(m, max_items, min_wg) <= it:
                a = m
            else:
                b = m
        out[it] = (lo, a)
        lo = a + 1
        it <<= 1
    return out


def lsd_gaps(n_act, n):
    """lsd_gaps with the default knobs: the LSD plan's last pass writes the offsets itself (the dense form)."""
    p = plan_of(n_act)
    return (not p.two_level) and sum(p.lsd[:-1]) <= 16 and n >= 2 * (n_act + 2)


# ---- batch builders (seeded; uint32 handles) --------------------------------------------------------------------
def alias_handles(n_act):
    """Handles that are not ORL_NO_ACT alone but must land in the unresolved bucket: every act >= n_act does."""
    w = bit_length(n_act)
    c = [n_act, n_act + 1, 1 << w, 0x80000000, 0xFFFFFFFE, NO_ACT]
    return np.array(sorted({x for x in c if n_act <= x < (1 << 32)}), np.uint32)


def uniform(n_act, n, seed, unresolved=0.05):
    """Uniform over [0, n_act), `unresolved` of the messages ORL_NO_ACT."""
    rng = np.random.default_rng([seed, n_act, n, 1])
    a = rng.integers(0, n_act, n, dtype=np.int64).astype(np.uint32)
    a[rng.random(n) < unresolved] = NO_ACT
    return a


def aliases(n_act, n, seed, unresolved=0.05):
    """Like uniform, but every unresolved message draws its handle from alias_handles(n_act)."""
    rng = np.random.default_rng([seed, n_act, n, 2])
    a = rng.integers(0, n_act, n, dtype=np.int64).astype(np.uint32)
    u = rng.random(n) < unresolved
    a[u] = rng.choice(alias_handles(n_act), int(u.sum()))
    return a


def edge_keys(n_act):
    """The keys (in [0, n_act], n_act = unresolved) at this width's edges: 0, 1, n_act - 1, both sides of every digit
    boundary of the plan, the first and last key of the first, a middle and the last top-digit bucket, n_act."""
    p = plan_of(n_act)
    keys = {0, 1, n_act - 1, n_act}
    if p.two_level:
        shifts = [p.lb] if p.hb > 0 else []
    else:
        shifts = list(np.cumsum(p.lsd)[:-1])
    for s in shifts:
        keys |= {(1 << int(s)) - 1, 1 << int(s)}
    if shifts:
        top = int(shifts[-1])
        last = n_act >> top  # the top-digit bucket of the largest key
        for b in (0, last // 2, last):
            keys |= {b << top, ((b + 1) << top) - 1}
    return np.array(sorted(k for k in keys if 0 <= k <= n_act), np.int64)


def _as_handles(keys, n_act):
    return np.where(keys >= n_act, NO_ACT, keys).astype(np.uint32)


def edges(n_act, n, seed):
    """Only edge_keys(n_act), shuffled (the unresolved bucket as ORL_NO_ACT)."""
    rng = np.random.default_rng([seed, n_act, n, 3])
    return _as_handles(rng.choice(edge_keys(n_act), n), n_act)


def one_key(n_act, n, which):
    """The whole batch in one bucket: which = "first" (0), "last" (n_act - 1) or "unresolved"."""
    k = {"first": 0, "last": n_act - 1, "unresolved": NO_ACT}[which]
    return np.full(n, k, np.uint32)


def far_keys(n_act, n, seed):
    """A few keys far apart, none of them the first, the last or the unresolved bucket: long runs of empty buckets
    before the first key, between keys and after the last one (the LSD plan's queued gaps)."""
    rng = np.random.default_rng([seed, n_act, n, 4])
    k = sorted({min(x, n_act - 1) for x in (5, 6, n_act // 2, n_act // 2 + 1, n_act - 1 - n_act // 5)})
    return rng.choice(np.array(k, np.uint32), n)


def hot_mix(n_act, n, seed, hot, count, unresolved=0.01):
    """uniform(), with `count` messages at random positions given the key `hot` (hot == n_act: mixed aliases)."""
    rng = np.random.default_rng([seed, n_act, n, 5])
    a = uniform(n_act, n, seed, unresolved)
    pos = rng.choice(n, count, replace=False)
    a[pos] = rng.choice(alias_handles(n_act), count) if hot >= n_act else np.uint32(hot)
    return a


BUILDERS = ("uniform", "edges", "one_first", "one_last", "one_unresolved", "aliases", "far")


def build(name, n_act, n, seed=4):
    if name == "uniform":
        return uniform(n_act, n, seed)
    if name == "aliases":
        return aliases(n_act, n, seed)
    if name == "edges":
        return edges(n_act, n, seed)
    if name == "far":
        return far_keys(n_act, n, seed)
    assert name.startswith("one_"), name
    return one_key(n_act, n, name[4:])


# ---- the width matrix of tests/test_gpu_stage4_widths.py ------------------------------------------------------
WIDTHS = tuple(range(1, 28))   # 28..31: the offsets array alone is 1 to 8 GB
SIZES = (1, 255, 4096, 4097, 3 * 4096 + 1, 40_001)
LSD_FIRST_W = 2 * K_MAX_DIGIT_BITS + 1


def width_cases():
    """Both edges of every width: n_act = 2^(w-1) (the unresolved key alone has the top bit) and 2^w - 1 (the
    unresolved key is all ones).  w = 1 has n_act = 1 only."""
    out = []
    for w in WIDTHS:
        for n_act in sorted({1 << (w - 1), (1 << w) - 1}):
            out.append((w, n_act))
    return out


def width_batches(n_act):
    """The (builder, n) list of one width case: every builder at every size; the far-apart keys on the LSD plan only
    (its offsets come from the gaps between sorted keys)."""
    two = plan_of(n_act).two_level
    return [(b, n) for b in BUILDERS if not (two and b == "far") for n in SIZES]


def dense_case():
    """The dense LSD form off the tested width 24: (n_act, n) with 23-bit keys and the smallest batch lsd_gaps takes."""
    n_act = 1 << 22
    return n_act, 2 * (n_act + 2) + 1000


ROUTE_WIDTHS = (11, 19, 23)    # one level, a two-level width no other test has, LSD


def route_cases():
    """(w, n_act, items, n): the route kernel as pass 0's producer, one batch size inside each route_items range (its
    first n; the last but 100 for items = 1), at one context per plan kind."""
    out = []
    for w in ROUTE_WIDTHS:
        n_act = (1 << w) - 1 if w != LSD_FIRST_W else 1 << (w - 1)
        for items, (lo, hi) in sorted(route_item_ranges(plan_of(n_act).max_items).items()):
            out.append((w, n_act, items, hi - 100 if items == 1 else lo))
    return out


HOT_WIDTHS = ((12, (1 << 12) - 1), (15, 1 << 14), (17, (1 << 17) - 1), (21, 1 << 20), (22, (1 << 22) - 1))
HOT_N = K_HOT_MIN_BATCH + 4097
