"""Stage 5 (CSR fan-out): the plan of one call restated on the CPU, degree families built for the kernels' own edges, and
the case lists that tests/test_gpu_fanout_edges.py runs (test infrastructure; no GPU needed, the library is never called).

The code restated is all in orleans_amd/csrc/route_kernels.hip: the degree scan's launch regimes
(launch_fanout_route_bucket / launch_fanout_expand), the publisher block map k_scan_down<.., WIDEN> writes (block_map),
fan_range with and without the map (fan_range, wave_find_pub), and the per-message upper_bound - 1 search over the
staged offsets or, past the LDS limit, over the offsets in global memory (plan).  Every constant is read from the
sources.  plan() returns the publisher the kernels would find for every emitted message and a record of the regimes
the call reaches; the GPU tests use the record to choose inputs and tests/test_fanout_ref.py asserts what their case
lists cover.  The expected outputs of the GPU tests never come from here: they are cpu_ref.fanout_expand and the
oracle's route and bucket.

  small_csr        a follower graph whose nodes have the prescribed degrees DEGREES (COPIES nodes of each, other targets)
  FAMILIES         named publisher lists over it (zeros_edges, zero_runs, ones, giants, block_aligned and its -1 / +1
                   forms, duplicates, random_mix)
  Form / Call      a context's table form and one fan-out call; regimes_of(call, form) is its plan's record
  *_calls()        the GPU file's case lists
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache
from typing import Optional

import numpy as np

import stage4_ref as S4

_K = S4._K
_const = S4._const
FAN_BLK_SHIFT = _const(_K, r"constexpr uint32_t kFanBlkShift = (\d+),")
FAN_BLK = 1 << FAN_BLK_SHIFT
FBLK_SERIAL = _const(_K, r"constexpr uint32_t kFblkSerial = (\d+);")
FAN_LDS = _const(_K, r"#define ORL_FAN_LDS (\d+)")
FAN_LDS_PF = FAN_LDS - _const(_K, r"return PF \? kFanLds - (\d+)u : kFanLds;")
SCAN_SMALL_CHUNK = _const(_K, r"constexpr uint32_t kScanSmallChunk = (\d+);")
SCAN_DIRECT_CHUNKS = _const(_K, r"constexpr uint32_t kScanDirectChunks = (\d+);")
SCAN_CHUNK = _const(_K, r"constexpr uint32_t kScanChunk = (\d+);")
SELF_SCAN_CHUNKS = _const(_K, r"constexpr uint32_t kSelfScanChunks = (\d+);")
SCAN_ROWS = _const(_K, r"constexpr uint32_t kScanRows = (\d+);")
FAN_MIN_WG = _const(_K, r"uint32_t fan_min_wgs\(\) \{[^}]*?return x > 0 \? \(uint32_t\)x : (\d+)u;")
EXPAND_MAX_ITEMS = _const(_K, r"const uint32_t items = route_items\(total, (\d+)\);")
WAVE = 64  # lanes: the wave-written map's round, the 64-way search
TILE0 = S4.K_ROUTE_THREADS * S4.K_ITEMS  # kTile: a context's max_batch is at least this

SPAN_REGIMES = tuple(f"span=={x}" for x in (FAN_LDS_PF, FAN_LDS_PF + 1, FAN_LDS, FAN_LDS + 1))
SCAN_REGIMES = ("scan_small_one_chunk:last", "scan_small:first", "scan_small:last", "scan_direct:first", "scan_direct:last",
                "scan_sums:first")
COL_REGIMES = ("self_cols", "no_self_cols", "self_cols:last_chunk_count", "no_self_cols:first_chunk_count",
               "col_chunk:full", "col_chunk:full+1")
REGIMES = ("in_lds", "global_search") + SPAN_REGIMES + (
    "fblk_serial", "fblk_serial:most", "fblk_wave", "fblk_wave:fewest", "fblk_wave_multi_round",
    "sentinel_on_block_boundary", "publisher_on_block_boundary", "first_tile_mid_nd", "wave_search", "zero_degree",
    "zero_degree_leading", "zero_degree_trailing") + SCAN_REGIMES + COL_REGIMES


def _ceil_div(a, b):
    return -(-a // b)


# ---- the plan of one call, restated ------------------------------------------------------------------------------
def offsets(deg):
    """The scanned degrees, poff[n_pub + 1] (relative to the fan-out); the scan is 32-bit."""
    poff = np.zeros(len(deg) + 1, np.int64)
    np.cumsum(np.asarray(deg, np.int64), out=poff[1:])
    assert poff[-1] < 1 << 32 and (np.asarray(deg, np.int64) < 1 << 32).all(), "the header's stage-5 precondition"
    return poff


def scan_regime(m):
    """The degree scan's launch regime for m = n_pub + 1 elements and the first / last m it holds for."""
    small_max = SCAN_SMALL_CHUNK * SCAN_DIRECT_CHUNKS
    if m <= small_max:
        return ("scan_small_one_chunk", 1, SCAN_SMALL_CHUNK) if m <= SCAN_SMALL_CHUNK else \
            ("scan_small", SCAN_SMALL_CHUNK + 1, small_max)
    if _ceil_div(m, SCAN_CHUNK) <= SCAN_DIRECT_CHUNKS:
        return "scan_direct", small_max + 1, SCAN_CHUNK * SCAN_DIRECT_CHUNKS
    return "scan_sums", SCAN_CHUNK * SCAN_DIRECT_CHUNKS + 1, None


def scan_regimes(m):
    name, first, last = scan_regime(m)
    out = {name}
    if m == first:
        out.add(name + ":first")
    if m == last:
        out.add(name + ":last")
    return out


def block_map(poff, fcap):
    """fblk[fcap] as k_scan_down<.., WIDEN> writes it, -1 where it writes nothing (whatever an earlier call left), and
    which of its write paths ran: publisher p owns the blocks k with poff[p] <= k * kFanBlk < poff[p + 1], at most
    kFblkSerial of them written by its own thread, more by the whole wave 64 at a time; the last element writes the
    sentinel fblk[ceil(total / kFanBlk)] = n_pub - 1."""
    n_pub = len(poff) - 1
    fblk = np.full(fcap, -1, np.int64)
    k0 = (poff[:-1] + FAN_BLK - 1) >> FAN_BLK_SHIFT
    k1 = np.minimum((poff[1:] + FAN_BLK - 1) >> FAN_BLK_SHIFT, fcap)
    cnt = np.maximum(k1 - k0, 0)
    tot = int(cnt.sum())
    within = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    fblk[np.repeat(k0, cnt) + within] = np.repeat(np.arange(n_pub, dtype=np.int64), cnt)
    ks = int((poff[-1] + FAN_BLK - 1) >> FAN_BLK_SHIFT)
    if n_pub >= 1 and ks < fcap:
        fblk[ks] = n_pub - 1
    paths = set()
    if ((cnt > 0) & (cnt <= FBLK_SERIAL)).any():
        paths.add("fblk_serial")
    if (cnt == FBLK_SERIAL).any():
        paths.add("fblk_serial:most")
    if (cnt > FBLK_SERIAL).any():
        paths.add("fblk_wave")
    if (cnt == FBLK_SERIAL + 1).any():
        paths.add("fblk_wave:fewest")
    if (cnt > WAVE).any():
        paths.add("fblk_wave_multi_round")
    return fblk, paths


def wave_find_pub(poff, n_pub, v):
    """wave_find_pub: the last p in [0, n_pub) with poff[p] <= v, by rounds of 64 evenly spaced samples."""
    lo, hi = 0, n_pub - 1
    lanes = np.arange(WAVE, dtype=np.int64)
    while lo < hi:
        step = (hi - lo + WAVE) // WAVE
        sl = np.minimum(lo + lanes * step, hi)
        le = poff[sl] <= v
        assert le[0] and not (np.diff(le.astype(np.int8)) > 0).any(), "the ballot is a prefix of lanes"
        top = int(np.nonzero(le)[0][-1])
        nlo = min(lo + top * step, hi)
        if top < WAVE - 1:
            nx = min(lo + (top + 1) * step, hi)
            if nx > nlo:
                hi = nx - 1
        lo = nlo
    return lo


def fan_range(poff, fblk, fb, fl, upper_plus_one=True):
    """fan_range: the publishers [p_lo, p_hi] of the tile whose first / last fan-out messages are fb / fl.
    upper_plus_one=False is a mutation (the upper block without its + 1) for tests/test_fanout_ref.py."""
    n_pub = len(poff) - 1
    if fblk is None:
        return wave_find_pub(poff, n_pub, fb), wave_find_pub(poff, n_pub, fl)
    kmax = int((poff[n_pub] + FAN_BLK - 1) >> FAN_BLK_SHIFT)
    ku = min((fl >> FAN_BLK_SHIFT) + (1 if upper_plus_one else 0), kmax)
    lo, hi = int(fblk[fb >> FAN_BLK_SHIFT]), int(fblk[ku])
    assert lo >= 0 and hi >= 0, "the tile reads a map entry this call's scan did not write"
    return lo, hi


@dataclass
class Plan:
    poff: np.ndarray            # int64[n_pub + 1], relative to the fan-out
    pub_of: np.ndarray          # int64[lim - nd]: the publisher found for every fan-out message below min(n, real)
    spans: list                 # per fan-out tile
    regimes: set = field(default_factory=set)
    used_map: bool = False


def plan(deg, nd=0, n=None, tile=S4.K_ROUTE_THREADS, limit=FAN_LDS, fcap=0, upper_plus_one=True):
    """One call: deg[n_pub] the publishes' out-degrees, nd direct messages in front, n the total the kernel is given
    (None: the scanned one), tile = kRouteThreads * items, limit = fan_lds_pubs of the kernel form, fcap = the block map's
    capacity for this call (0: the context has none)."""
    deg = np.asarray(deg, np.int64)
    n_pub = len(deg)
    poff = offsets(deg)
    real = nd + int(poff[-1])
    n = real if n is None else n
    lim = min(n, real)
    use_map = bool(fcap) and _ceil_div(n, FAN_BLK) < fcap
    fblk, paths = block_map(poff, fcap) if use_map else (None, set())
    out = Plan(poff, np.full(max(lim - nd, 0), -1, np.int64), [], set(paths), use_map)
    reg = out.regimes
    reg |= scan_regimes(n_pub + 1)
    nz = np.nonzero(deg)[0]
    if lim > nd and len(nz) < n_pub:
        reg.add("zero_degree")
        if nz[0] > 0:
            reg.add("zero_degree_leading")
        if nz[-1] < n_pub - 1:
            reg.add("zero_degree_trailing")
    for t in range(_ceil_div(n, tile) if n else 0):
        base = t * tile
        last = (lim if lim - base < tile else base + tile) - 1
        fbase = max(base, nd)
        if not (base < lim and last >= nd):
            continue
        fb, fl = fbase - nd, last - nd
        p_lo, p_hi = fan_range(poff, fblk, fb, fl, upper_plus_one)
        span = p_hi - p_lo + 1
        out.spans.append(span)
        f = np.arange(fb, fl + 1, dtype=np.int64)
        if span <= limit:  # fan_stage: poff[p_lo .. p_lo + span] in LDS, the search over all span + 1 of them
            assert p_lo + span <= n_pub, "fan_stage reads past poff[n_pub]"
            reg.add("in_lds")
            pq = p_lo + np.searchsorted(poff[p_lo:p_lo + span + 1], f, side="right") - 1
        else:              # the search over poff[p_lo .. p_hi] in global memory
            reg.add("global_search")
            pq = p_lo + np.searchsorted(poff[p_lo:p_hi + 1], f, side="right") - 1
        out.pub_of[fb:fl + 1] = pq
        if f"span=={span}" in SPAN_REGIMES and span in (limit, limit + 1):
            reg.add(f"span=={span}")
        if use_map:
            kmax = int((poff[n_pub] + FAN_BLK - 1) >> FAN_BLK_SHIFT)
            if poff[n_pub] % FAN_BLK == 0 and (fl >> FAN_BLK_SHIFT) + 1 >= kmax:
                reg.add("sentinel_on_block_boundary")
        else:
            reg.add("wave_search")
        if base < nd:
            reg.add("first_tile_mid_nd")
    if use_map and lim > nd:
        starts = poff[:-1][(deg > 0) & (poff[:-1] > 0) & (poff[:-1] < lim - nd)]
        if (starts % FAN_BLK == 0).any():
            reg.add("publisher_on_block_boundary")
    return out


def brute_pub_of(deg, nd=0, n=None):
    """The publisher of every fan-out message, brute force."""
    deg = np.asarray(deg, np.int64)
    full = np.repeat(np.arange(len(deg), dtype=np.int64), deg)
    return full if n is None else full[:max(min(n, nd + len(full)) - nd, 0)]


def self_cols(n, n_act, max_batch, items):
    """launch_fanout_route_bucket's self-summed columns: (on, chunks of kScanRows tiles, the most chunks it is on for);
    None when the route kernel builds no histogram (one-level plan)."""
    p = S4.plan_of(n_act)
    assert p.two_level, "the LSD plan's histogram digit is not restated here"
    if p.hb == 0:
        return None
    mb = max(max_batch, TILE0)
    most = min(_ceil_div(_ceil_div(mb, S4.K_ROUTE_THREADS), SCAN_ROWS), SELF_SCAN_CHUNKS)
    nch = _ceil_div(_ceil_div(n, S4.K_ROUTE_THREADS * items), SCAN_ROWS)
    return nch <= most, nch, most


# ---- the follower graph ----------------------------------------------------------------------------------------------
DEGREES = (0, 1, 2, 255, 256, 257, 2048, 2049, 16_641, 70_000)
COPIES = 2
N_FOLLOWERS = 3000     # follower ids: [0, 1500) registered, [1500, 2000) registered then removed, the rest never


def node(deg, copy=0):
    """The CSR node with out-degree deg (copy < COPIES: same degree, other followers)."""
    return copy * len(DEGREES) + DEGREES.index(deg)


@lru_cache(maxsize=None)
def small_csr(seed=5):
    """(csr_off uint64[n_nodes + 1], csr_tgt uint32, node degrees): COPIES nodes of every degree of DEGREES and a last
    node of degree 0 (the offsets end in a repeat)."""
    node_deg = np.array(list(DEGREES) * COPIES + [0], np.int64)
    off = np.zeros(len(node_deg) + 1, np.uint64)
    off[1:] = np.cumsum(node_deg)
    rng = np.random.default_rng(seed)
    tgt = rng.integers(0, N_FOLLOWERS, int(off[-1]), dtype=np.int64).astype(np.uint32)
    for a in (off, tgt, node_deg):
        a.setflags(write=False)
    return off, tgt, node_deg


Z = (node(0, 0), node(0, 1), len(DEGREES) * COPIES)  # the zero-degree nodes: the first one, a middle one, the last one


def _zeros(k, start=0):
    return [Z[(start + i) % len(Z)] for i in range(k)]


def degrees_of(pubs):
    return small_csr()[2][np.asarray(pubs, np.int64)]


def zeros_edges():
    """Leading and trailing zero runs around a few publishers."""
    return _zeros(300) + [node(1), node(257), node(2, 1), node(255)] + _zeros(5, 1) + [node(256, 1)] + _zeros(700, 2)


ZERO_RUN_SPANS = (FAN_LDS_PF, FAN_LDS_PF + 1, FAN_LDS, FAN_LDS + 1, 30_002)


def zero_runs():
    """Pairs of non-zero publishers separated by runs of zeros.  With tiles of kFanBlk messages and no direct message, a
    publisher of kFanBlk followers fills tile t, so fan_range gives p_lo = it and p_hi = the next non-zero publisher: a run
    of S - 2 zeros between them is a span of S, for S in ZERO_RUN_SPANS (both LDS limits, one more, and far beyond); then
    runs around degrees that are no multiple of the block."""
    out = []
    for i, s in enumerate(ZERO_RUN_SPANS):
        out += [node(FAN_BLK, i % COPIES)] + _zeros(s - 2, i)
    out += [node(FAN_BLK, 1)]
    out += [node(255)] + _zeros(100) + [node(1, 1)] + _zeros(FAN_LDS_PF - 1) + [node(2)] + _zeros(FAN_LDS - 1, 1)
    out += [node(257, 1)] + _zeros(40, 2)
    return out


def ones():
    return [node(1, i % COPIES) for i in range(2049)]


def giants():
    """Degrees 2048, 2049, 16 641 and 70 000, each flanked by zeros: a publisher of exactly kFblkSerial blocks, one of one
    more (the first the wave writes), one of 65 blocks + 1 (a second round of the wave loop) and one of 273."""
    out = []
    for i, d in enumerate((2048, 2049, 16_641, 70_000)):
        out += _zeros(3, i) + [node(d, i % COPIES)] + _zeros(2, i + 1)
    return out


def block_aligned(delta=0):
    """Multiples of the block only, so every publisher starts on a block and the total is a multiple of it (the sentinel
    block is a block of its own); delta = -1 / +1: the last publisher one follower short / over."""
    last = {0: 256, -1: 255, 1: 257}[delta]
    return ([node(256)] + _zeros(2) + [node(2048, 1)] + [node(256, 1)] + _zeros(1, 1) + [node(2048)] + _zeros(7, 2)
            + [node(last, 1)] + _zeros(3))


def duplicates():
    """One account published many times in a row."""
    return [node(257)] * 40 + [node(2)] * 600 + [Z[1]] * 50 + [node(2048, 1)] * 3 + [Z[2]] * 2 + [node(1)] * 300


def random_mix(seed=11, n_pub=420):
    """All of the above drawn at random, at least 30 % zeros."""
    rng = np.random.default_rng(seed)
    degs = np.array([1, 2, 255, 256, 257, 2048, 2049], np.int64)
    w = np.array([6, 6, 4, 4, 4, 1, 1], np.float64)
    out = []
    for i in range(n_pub):
        if rng.random() < 0.4:
            out.append(Z[int(rng.integers(0, len(Z)))])
        else:
            out.append(node(int(rng.choice(degs, p=w / w.sum())), int(rng.integers(0, COPIES))))
    out[n_pub // 3] = node(16_641)
    out[n_pub // 2] = out[n_pub // 2 + 1] = node(257, 1)
    return out


FAMILIES = {"zeros_edges": zeros_edges, "zero_runs": zero_runs, "ones": ones, "giants": giants,
            "block_aligned": block_aligned, "block_aligned-1": lambda: block_aligned(-1),
            "block_aligned+1": lambda: block_aligned(1), "duplicates": duplicates, "random_mix": random_mix}


@lru_cache(maxsize=None)
def family(name):
    p = np.array(FAMILIES[name](), np.uint32)
    p.setflags(write=False)
    return p


def exact_total(total, zeros_between=3):
    """Publishers emitting exactly `total` messages: the largest degrees first, zeros between them."""
    out, left, i = _zeros(2), total, 0
    for d in sorted((x for x in DEGREES if x), reverse=True):
        while left >= d:
            out += [node(d, i % COPIES)] + _zeros(zeros_between, i)
            left -= d
            i += 1
    assert left == 0
    return np.array(out, np.uint32)


def many_zeros(n_giants=30, n_zero=100_000):
    """n_giants publishers of 70 000 followers among n_zero zero-degree ones."""
    out = np.array(_zeros(n_zero + n_giants), np.uint32)
    at = np.linspace(17, n_zero + n_giants - 29, n_giants).astype(np.int64)
    out[at] = [node(70_000, i % COPIES) for i in range(n_giants)]
    return out


def sparse_pubs(n_pub):
    """The scan-regime batches: n_pub publishes, all of degree zero but a few at the chunk edges and the two ends."""
    out = np.array(_zeros(n_pub), np.uint32) if n_pub < 4096 else np.resize(np.array(Z, np.uint32), n_pub)
    degs = (257, 1, 2048, 2, 255, 256)
    for i, at in enumerate((1023, 1024, 4095, 4096, n_pub - 2, n_pub - 1)):
        if 0 <= at < n_pub:
            out[at] = node(degs[i], i % COPIES)
    return out


def all_zero(n_pub):
    return np.resize(np.array(Z, np.uint32), n_pub)


def single(k):
    """One follower in all: k zero-degree publishes, one of degree 1, k more."""
    return np.array(_zeros(k) + [node(1, 1)] + _zeros(k, 1), np.uint32)


def wave_pubs(extra):
    """The wave-search batches (4352 + extra messages): both searched values of the tile [2048, 2304) fall after zero
    runs, and its span is beyond the LDS limit."""
    out = (_zeros(700) + [node(255)] + _zeros(10, 1) + [node(2048)] + _zeros(1100, 2) + [node(2049, 1)] + _zeros(900))
    return np.array(out + [node(1)] * extra + _zeros(64, 1), np.uint32)


# ---- the GPU file's cases ------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Form:
    """A context: how its table form is selected, the fan-out kernel's LDS limit there, and its sizes."""
    name: str
    probe_form: int             # Q_PROBE_FORM
    env: tuple                  # ((name, value or None = unset), ...) at orl_ctx_create
    guid_grain: bool            # a Guid-keyed grain registered: no probe table, the PW 0 kernel with its prefetch
    n_act: int = (1 << 11) - 1
    max_batch: int = 1 << 18

    @property
    def limit(self):
        return FAN_LDS_PF if self.probe_form == 32 else FAN_LDS

    def at(self, n_act=None, max_batch=None):
        return Form(self.name, self.probe_form, self.env, self.guid_grain, n_act or self.n_act, max_batch or self.max_batch)


_E8 = (("ORL_NO_PROBE8", "0"), ("ORL_NO_PROBE16", "0"), ("ORL_FAN_U", None))
FORMS = (Form("8B", 8, _E8, False),
         Form("16B", 16, (("ORL_NO_PROBE8", "1"), ("ORL_NO_PROBE16", "0"), ("ORL_FAN_U", None)), False),
         Form("16B-U2", 16, (("ORL_NO_PROBE8", "1"), ("ORL_NO_PROBE16", "0"), ("ORL_FAN_U", "2")), False),
         Form("16B-U4", 16, (("ORL_NO_PROBE8", "1"), ("ORL_NO_PROBE16", "0"), ("ORL_FAN_U", "4")), False),
         Form("32B", 32, _E8, True))
FORM = {f.name: f for f in FORMS}
# stage4_ref.ROUTE_WIDTHS' one-level and two-level widths, n_act as route_cases() takes it
ROUTE_N_ACT = tuple((1 << w) - 1 for w in S4.ROUTE_WIDTHS[:2])
COL_N_ACT = 1 << 11            # 12 bits: two levels, so the fan-out kernel builds the first digit's histogram
OVERS = (1, 255, 256, 777)
ROUTE_ND = (0, 1, 257, 700)


@dataclass(frozen=True)
class Call:
    """One fan-out call.  entry: device / keys / mixed (the three route entry points) or expand; keyed: followers through
    the key table; total: None = read back, 0 = ORL_OPT_TOTAL_GIVEN exact, k > 0 = overstated by k, k < 0 = understated."""
    pubs_of: str                # a name of BUILDERS: a family, or a sized builder with its size in arg
    entry: str = "device"
    nd: int = 0
    keyed: bool = False
    total: Optional[int] = None
    cap: int = 0                # expand: the output buffer's records (0: the total + 64)
    arg: Optional[int] = None

    @property
    def source(self):
        """(builder, size): what the publisher list, and so every reference of it, is keyed by."""
        return self.pubs_of, self.arg

    @property
    def pubs(self):
        return _pubs(self.pubs_of, self.arg)

    @property
    def id(self):
        t = "read" if self.total is None else "exact" if self.total == 0 else f"{self.total:+d}"
        src = self.pubs_of if self.arg is None else f"{self.pubs_of}({self.arg})"
        return f"{src}-{self.entry}{'-keyed' if self.keyed else ''}-nd{self.nd}-{t}"


BUILDERS = dict(FAMILIES, exact_total=exact_total, many_zeros=many_zeros, sparse_pubs=sparse_pubs, wave_pubs=wave_pubs,
                all_zero=all_zero, single=single)


@lru_cache(maxsize=None)
def _pubs(name, arg):
    p = np.asarray(BUILDERS[name]() if arg is None else BUILDERS[name](arg), np.uint32)
    p.setflags(write=False)
    return p


# (entry, nd, keyed): every route entry point, nd > 0 through the mixed form
ROUTE_COMBOS = (("device", 0, False), ("keys", 0, True), ("mixed", 1, False), ("mixed", 257, True), ("mixed", 700, False))


def route_calls():
    """Every family x ROUTE_COMBOS with the total read back, and every family x (exact, OVERS) with the combo rotating, so
    every family meets every total mode and every combo meets every total mode."""
    out = []
    for fam in FAMILIES:
        for entry, nd, keyed in ROUTE_COMBOS:
            out.append(Call(fam, entry, nd, keyed, None))
    for i, fam in enumerate(FAMILIES):
        for j, tot in enumerate((0,) + OVERS):
            entry, nd, keyed = ROUTE_COMBOS[(i + j) % len(ROUTE_COMBOS)]
            out.append(Call(fam, entry, nd, keyed, tot))
    return out


def n_of(call):
    """(real total, the n the call passes or gets back)."""
    real = call.nd + int(degrees_of(call.pubs).sum())
    return real, real if call.total is None else real + call.total


def items_of(call, form):
    n = n_of(call)[1]
    if call.entry == "expand":
        return S4.route_items(n, EXPAND_MAX_ITEMS)
    return S4.route_items(n, S4.plan_of(form.n_act).max_items, FAN_MIN_WG)


def fcap_of(call, form):
    mb = max(form.max_batch, TILE0)
    blk_cap = _ceil_div(mb, FAN_BLK) + 2
    out_cap = (call.cap or n_of(call)[1] + 64) if call.entry == "expand" else mb
    return min(_ceil_div(out_cap, FAN_BLK) + 1, blk_cap)


def plan_of_call(call, form, **kw):
    real, n = n_of(call)
    if n == 0:
        return Plan(offsets(degrees_of(call.pubs)), np.zeros(0, np.int64), [], scan_regimes(len(call.pubs) + 1))
    items = items_of(call, form)
    limit = FAN_LDS if call.entry == "expand" else form.limit
    p = plan(degrees_of(call.pubs), call.nd, n, S4.K_ROUTE_THREADS * items, limit, fcap_of(call, form), **kw)
    if call.entry != "expand":
        sc = self_cols(n, form.n_act, form.max_batch, items)
        if sc is not None:
            on, nch, most = sc
            p.regimes.add("self_cols" if on else "no_self_cols")
            if on and nch == most:
                p.regimes.add("self_cols:last_chunk_count")
            if not on and nch == most + 1:
                p.regimes.add("no_self_cols:first_chunk_count")
            tiles = _ceil_div(n, S4.K_ROUTE_THREADS * items)
            if tiles == SCAN_ROWS:
                p.regimes.add("col_chunk:full")
            if tiles == SCAN_ROWS + 1:
                p.regimes.add("col_chunk:full+1")
    return p


def regimes_of(call, form):
    return plan_of_call(call, form).regimes


def degenerate_calls():
    """n_pub = 0; every degree zero without and with direct messages; a total of exactly 1 (one follower, and one direct
    message alone)."""
    return [Call("all_zero", "device", arg=0), Call("all_zero", "mixed", 700, arg=0), Call("all_zero", "mixed", 1, arg=0),
            Call("all_zero", "device", arg=900), Call("all_zero", "keys", 0, True, arg=900),
            Call("all_zero", "device", total=0, arg=900), Call("all_zero", "mixed", 700, True, arg=1025),
            Call("all_zero", "mixed", 1, arg=300), Call("single", "device", arg=500),
            Call("single", "keys", 0, True, total=0, arg=500), Call("single", "device", total=255, arg=0)]


# back-to-back on one context: a stale block map and stale self-summed columns must not show
SEQUENCE = ("giants", "zero_runs", "giants", "ones", "block_aligned", "giants")
COL_TOTALS = (SCAN_ROWS * S4.K_ROUTE_THREADS, SCAN_ROWS * S4.K_ROUTE_THREADS + 1,
              SELF_SCAN_CHUNKS * SCAN_ROWS * S4.K_ROUTE_THREADS, SELF_SCAN_CHUNKS * SCAN_ROWS * S4.K_ROUTE_THREADS + 1)
COL_MAX_BATCH = 2_200_000
COL_FORMS = tuple(FORM[k].at(COL_N_ACT, COL_MAX_BATCH) for k in ("8B", "32B"))


def col_calls():
    return [Call("exact_total", arg=t) for t in COL_TOTALS] + [Call("many_zeros")]


UNDERSTATED = (Call("giants", "device", total=-300), Call("zero_runs", "keys", 0, True, total=-257),
               Call("giants", "mixed", 700, total=-1), Call("zero_runs", "expand", total=-256),
               Call("giants", "mixed", 257, True, total=-(2048 + 2049 + 16_641 + 70_000)))  # the direct messages alone

EXPAND_FORM = FORM["8B"].at(16, 1 << 18)
WAVE_FORM = FORM["8B"].at(16, TILE0)       # fan_blk_cap = max_batch / kFanBlk + 2: a cap beyond it clamps the map
WAVE_CAP = 20_000
SCAN_M = (1, 2, SCAN_SMALL_CHUNK, SCAN_SMALL_CHUNK + 1, SCAN_SMALL_CHUNK * SCAN_DIRECT_CHUNKS,
          SCAN_SMALL_CHUNK * SCAN_DIRECT_CHUNKS + 1, SCAN_CHUNK * SCAN_DIRECT_CHUNKS, SCAN_CHUNK * SCAN_DIRECT_CHUNKS + 1)
SCAN_FORM = FORM["8B"].at(16, SCAN_M[-1] + 4096)


def expand_calls():
    out = []
    for i, fam in enumerate(FAMILIES):
        out.append(Call(fam, "expand", keyed=False))
        out.append(Call(fam, "expand", keyed=True, total=((0,) + OVERS)[i % 5]))
        out.append(Call(fam, "expand", keyed=bool(i & 1), total=((0,) + OVERS)[(i + 2) % 5]))
    return out


def wave_calls():
    """Totals of 17 blocks (the clamped map of 18 entries still covers them) and 17 blocks + 1 (it does not)."""
    return [Call("wave_pubs", "expand", keyed=k, total=t, cap=WAVE_CAP, arg=x)
            for x in (0, 1) for k, t in ((False, None), (True, 0), (False, 777))]


def scan_calls():
    return [Call("sparse_pubs", "expand", keyed=(i % 3 == 2), arg=m - 1) for i, m in enumerate(SCAN_M)]


def groups():
    """{test of tests/test_gpu_fanout_edges.py: [(form, calls on one context of it, in order)]}."""
    under = [c for c in UNDERSTATED if c.entry != "expand"]
    return {
        "route": [(f.at(n_act), route_calls()) for n_act in ROUTE_N_ACT for f in FORMS],
        "degenerate": [(FORM["8B"].at(ROUTE_N_ACT[1]), degenerate_calls()), (FORM["32B"].at(ROUTE_N_ACT[0]), degenerate_calls())],
        "sequence": [(FORM[k].at(COL_N_ACT), [Call(fam) for fam in SEQUENCE]) for k in ("8B", "32B")],
        "col": [(f, col_calls()) for f in COL_FORMS],
        "understated": [(FORM["8B"].at(ROUTE_N_ACT[1]), under), (FORM["32B"].at(ROUTE_N_ACT[1]), under),
                        (EXPAND_FORM, [c for c in UNDERSTATED if c.entry == "expand"])],
        "expand": [(EXPAND_FORM, expand_calls())],
        "wave": [(WAVE_FORM, wave_calls())],
        "scan": [(SCAN_FORM, scan_calls())],
    }


def all_gpu_cases():
    """(call, form) of everything tests/test_gpu_fanout_edges.py runs."""
    return [(c, f) for g in groups().values() for f, calls in g for c in calls]
