"""The wire codec's machinery on the device: the pipelined kernels' window, held-row and big[] boundaries at every start
alignment, held batches of every size, waves that walk two and three chunks, the held list's overflow, the deferred
kernels (through LDS and from HBM), the form threshold, the buffer's end, and headers cut short whose neighbouring bytes
would complete them.

The inputs and case lists are tests/wire_pipe_ref.py's (tests/test_wire_pipe_ref.py asserts, without a GPU, which
regimes they reach at 8, 64, 256 and 304 CUs).  Every test first asserts that the plan for this device's CU count reaches
the regime it is about, and fails if it does not.  The expected outputs are oracle/wire_codec.py's, memoised per distinct
frame.  Every case runs decode_frames_device (sender from the header, and overridden) and stamp_frames_device, and every
comparison is exact: status, the 32-byte records and n_bad; status, output offsets, total and each frame's bytes.  The
outputs are pre-filled with a sentinel byte: a frame no pass wrote shows as sentinel bytes, and everything at and past
the total must still be the sentinel (the padding inside a frame's aligned size is not asserted).

No case passes an offset array, a route / activation array or an output buffer shorter than the call is told; none is
meant to make the device fault.
"""
import time

import numpy as np
import pytest

import wire_corpus as C
import wire_pipe_ref as R
from orleans_amd import _lib as L
from orleans_amd.engine import GrainDirectoryEngine

pytestmark = pytest.mark.gpu

SENT = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need an MI355X"
    return t


class World:
    def __init__(self, t):
        self.t = t
        self.cus = int(t.cuda.get_device_properties(0).multi_processor_count)
        self.eng = GrainDirectoryEngine(n_act=16, dir_capacity=16, max_batch=1024, device=0)
        self.eng.set_silos(R.N_SILOS)
        for s in range(R.N_SILOS):
            self.eng.set_silo_address(s, *C.silo_addr(s))
        for code, name in R.GRAIN_TYPES.items():
            self.eng.set_grain_type(code, name)
        kd = np.zeros(R.N_ACT_KEYS, L.KEY_DTYPE)
        kd["tcd"], kd["n0"], kd["n1"] = [k.tcd for k in R.ACT_KEYS], [k.n0 for k in R.ACT_KEYS], [k.n1 for k in R.ACT_KEYS]
        self.d_keys = t.from_numpy(kd.view(np.uint8)).cuda()
        self.stream = t.cuda.current_stream().cuda_stream
        self._cases = {}
        self._dev = (None, None)

    def case(self, name, make):
        """A case and its device inputs, built once; the device copy of one case at a time."""
        if name not in self._cases:
            self._cases[name] = make()
        return self._cases[name]

    def upload(self, case):
        if self._dev[0] is not case:
            t, p = self.t, case.pack()
            self._dev = (case, dict(
                buf=t.from_numpy(p.buf).cuda(), off=t.from_numpy(p.offs.view(np.int64)).cuda(),
                route=t.from_numpy(p.route.view(np.int32)).cuda(), act=t.from_numpy(p.act.view(np.int32)).cuda(),
                new=t.from_numpy(np.ascontiguousarray(p.new_keys).view(np.uint8).reshape(-1)).cuda()))
        return self._dev[1]

    def decode(self, case, n, so, nbytes=None):
        t, d = self.t, self.upload(case)
        d_out = t.full((max(n, 1), 32), SENT, dtype=t.uint8, device="cuda")
        d_st = t.full((max(n, 1),), SENT, dtype=t.uint8, device="cuda")
        d_bad = t.full((1,), -1, dtype=t.int32, device="cuda")
        self.eng.decode_frames_device(d["buf"], case.pack().nbytes if nbytes is None else nbytes, d["off"], n, d_out, d_st, d_bad,
                                      sender_override=so, stream=self.stream)
        t.cuda.synchronize()
        return d_st.cpu().numpy()[:n], d_out.cpu().numpy().reshape(-1).view(L.MSG_DTYPE)[:n], int(d_bad.cpu()[0])

    def stamp(self, case, n, alloc, out_cap, nbytes=None):
        t, d = self.t, self.upload(case)
        d_out = t.full((alloc,), SENT, dtype=t.uint8, device="cuda")
        d_ooff = t.full((max(n, 1),), -1, dtype=t.int64, device="cuda")
        d_tot = t.full((1,), -1, dtype=t.int64, device="cuda")
        d_st = t.full((max(n, 1),), SENT, dtype=t.uint8, device="cuda")
        self.eng.stamp_frames_device(d["buf"], case.pack().nbytes if nbytes is None else nbytes, d["off"], n, d["route"], d["act"],
                                     self.d_keys, R.N_ACT_KEYS, d["new"], d_out, out_cap, d_ooff, d_tot, d_st, stream=self.stream)
        t.cuda.synchronize()
        return d_st.cpu().numpy()[:n], d_ooff.cpu().numpy().view(np.uint64)[:n], int(d_tot.cpu()[0]), d_out.cpu().numpy()


@pytest.fixture(scope="module")
def world(torch):
    w = World(torch)
    yield w
    w.eng.close()


def _first(mask):
    return np.nonzero(mask)[0][:8].tolist()


def check_decode(world, case, n=None):
    n = case.n if n is None else n
    out = {}
    for so in (L.SENDER_FROM_HEADER, 3):
        st_ref, rec_ref, _ = case.expect_decode(so)
        st_ref, rec_ref = st_ref[:n], rec_ref[:n]
        st, rec, n_bad = world.decode(case, n, so)
        bad = st != st_ref
        assert not bad.any(), (case.name, n, so, "status", _first(bad), st[bad][:8], st_ref[bad][:8])
        bad = (rec.view(np.uint8).reshape(n, 32) != rec_ref.view(np.uint8).reshape(n, 32)).any(axis=1)
        assert not bad.any(), (case.name, n, so, "record", _first(bad))
        assert n_bad == int((st_ref != 0).sum())
        out[so] = (st, rec)
    return out


def check_stamp(world, case, n=None):
    n = case.n if n is None else n
    st_ref, sizes, off_ref, _, exp, msk = case.expect_stamp()
    st_ref, sizes, off_ref = st_ref[:n], sizes[:n], off_ref[:n]
    total = int(sizes.sum())
    st, off, tot, out = world.stamp(case, n, total + 1024, total + 1024)
    bad = off != off_ref
    assert not bad.any(), (case.name, n, "offsets", _first(bad))
    assert tot == total
    bad = st != st_ref
    assert not bad.any(), (case.name, n, "status", _first(bad), st[bad][:8], st_ref[bad][:8])
    wrong = (out[:total] != exp[:total]) & msk[:total]
    if wrong.any():
        b = int(np.nonzero(wrong)[0][0])
        i = int(np.searchsorted(off_ref, b, side="right")) - 1
        raise AssertionError((case.name, n, "bytes of frame", i, "at", b - int(off_ref[i]), "status", int(st_ref[i]),
                              "got", int(out[b]), "sentinel" if out[b] == SENT else "", "wrong bytes", int(wrong.sum())))
    assert (out[total:] == SENT).all(), "bytes at or past the total were written"
    return st, out[:total]


def check_both(world, case, n=None):
    t0 = time.perf_counter()
    d = check_decode(world, case, n)
    t1 = time.perf_counter()
    s = check_stamp(world, case, n)
    print("%s n=%d: decode checked in %.2f s, stamp in %.2f s" % (case.name, case.n if n is None else n, t1 - t0,
                                                                  time.perf_counter() - t1))
    return d, s


def report(name, pl, **extra):
    c = pl.counts()
    c.update(form="pipelined" if pl.pipelined else "simple", blocks=pl.blocks, chunks_per_wave_max=len(pl.wave_chunks(0)),
             surely_held=int(pl.surely_held.sum()), surely_deferred=int(pl.surely_deferred.sum()),
             overflowing_waves=len(pl.overflowing), **extra)
    print("reach %s: %s" % (name, c))


def test_window_boundary(world):
    """a. q0 + 8 + hl in {255, 256, 257} at every q0, filler last and TARGET_GRAIN last, pipelined and on a 300-frame
    prefix (the simple form)."""
    case = world.case("window", lambda: R.case_window(world.cus))
    p, pl = case.pack(), case.plan(world.cus)
    s = (p.offs & np.uint64(3)).astype(np.int64) + 8 + p.hls
    assert pl.pipelined and not case.plan(world.cus, 300).pipelined
    for n in (case.n, 300):
        for q in range(4):
            at = ((p.offs & np.uint64(3)) == q)[:n]
            assert all((at & (s[:n] == tot)).sum() >= 2 for tot in (255, 256, 257)), (n, q)
            assert (pl.cls[:n][at & (s[:n] <= 256)] == R.WINDOW).all() and (pl.cls[:n][at & (s[:n] == 257)] == R.HELD_FITS).all()
        assert n == 300 or all((pl.surely_held & (s == 257) & ((p.offs & np.uint64(3)) == q)).any() for q in range(4))
    report("window", pl)
    check_both(world, case)
    check_both(world, case, 300)


def test_held_and_long_boundaries(world):
    """b. fw in {259, 260, 261} and nw in {1023, 1024, 1025} words at every q0, a 20,000-byte header, every stamp status
    and the free-slot reuse form at a held, a big[] and an HBM length; out_cap falling inside a held and a deferred
    frame."""
    case = world.case("bounds", lambda: R.case_bounds(world.cus))
    p, pl = case.pack(), case.plan(world.cus)
    assert pl.pipelined and len(pl.overflowing) == 0
    fw = R.frame_words(p.offs.astype(np.int64) & 3, p.hls)
    for q in range(4):
        at = (p.offs & np.uint64(3)) == q
        for words, want in ((259, R.HELD_FITS), (260, R.HELD_FITS), (261, R.TOO_LONG_LDS), (1023, R.TOO_LONG_LDS),
                            (1024, R.TOO_LONG_LDS), (1025, R.TOO_LONG_HBM)):
            hit = at & (fw == words)
            assert hit.any() and (pl.cls[hit] == want).all(), (q, words)
            assert want != R.HELD_FITS or (hit & pl.surely_held).any()
    assert (p.hls == R.HUGE).any()
    st_ref = case.expect_stamp()[0]
    for hl, want in zip(R.STAMP_LENGTHS, (R.HELD_FITS, R.TOO_LONG_LDS, R.TOO_LONG_HBM)):
        hit = p.hls == hl
        assert (pl.cls[hit] == want).all() and len(set(case.eidx[hit].tolist())) == len(R.STAMP_FORM_STATUS)
        assert set(st_ref[hit].tolist()) == {L.STAMP_OK, L.STAMP_COMPLETE, L.STAMP_SKIPPED, L.STAMP_UNSUPPORTED, L.STAMP_MALFORMED}
    report("bounds", pl)
    check_both(world, case)
    # out_cap inside a held frame and inside a deferred frame
    _, sizes, off_ref, total, exp, msk = case.expect_stamp()
    ok = st_ref == L.STAMP_OK
    for j in (int(np.nonzero(pl.surely_held & ok & (p.hls == R.STAMP_LENGTHS[0]))[0][0]),
              int(np.nonzero(pl.surely_deferred & ok & (p.hls == R.STAMP_LENGTHS[1]))[0][0])):
        cut = int(off_ref[j])
        cap = cut + int(sizes[j]) // 2
        assert j > 64 and (sizes > 0).all()
        st, off, tot, out = world.stamp(case, case.n, (cap + 64 + 3) // 4 * 4, cap)
        np.testing.assert_array_equal(off, off_ref)
        assert tot == total
        np.testing.assert_array_equal(st[:j], st_ref[:j])
        assert (st[j:] == L.STAMP_OVERFLOW).all()
        assert not ((out[:cut] != exp[:cut]) & msk[:cut]).any()
        assert (out[cap:] == SENT).all(), "bytes past out_cap were written"


def test_held_batches(world):
    """c. One chunk per wave; chunks with exactly 0, 1, 15, 16, 17, 32, 33, 63 and 64 long headers at their first and
    last lanes; neighbouring held rows differ in length, alignment and content."""
    case = world.case("batches", lambda: R.case_batches(world.cus))
    pl = case.plan(world.cus)
    assert pl.pipelined and len(pl.overflowing) == 0 and case.n == 65536 + 64
    assert set(R.HELD_COUNTS) <= set(pl.wave_long[:pl.n_waves].tolist())
    assert all(sum(pl.chunk_long[c] > 0 for c in pl.wave_chunks(w)) <= 1 for w in range(pl.n_waves))
    assert int(pl.surely_held.sum()) == int(pl.long.sum()) > 0
    report("batches", pl, held_per_wave={k: int((pl.wave_long[:pl.n_waves] == k).sum()) for k in R.HELD_COUNTS})
    check_both(world, case)


def _walk(world):
    case = world.case("walk", lambda: R.case_walk(world.cus))
    pl = case.plan(world.cus)
    ch = pl.wave_chunks(0)
    assert pl.pipelined and pl.stride == 8 * world.cus
    assert len(ch) >= 3 and pl.n - ch[-1] * 64 == 1, "wave 0 walks three chunks, the last one a single frame"
    assert world.cus < 64 or (len(ch) == 3 and case.n == 2 * pl.stride * 64 + 1)
    for w, (c0, c1) in R.WALK_WAVES.items():
        assert [int(pl.chunk_long[c]) for c in pl.wave_chunks(w)[:2]] == [c0, c1] and pl.min_deferred[w] == max(c0 + c1 - 64, 0)
    assert pl.overflowing.tolist() == R.WALK_OVERFLOWING and pl.surely_held.sum() >= 20
    assert (pl.cls == R.TOO_LONG_LDS).any() and (pl.cls == R.TOO_LONG_HBM).any()
    return case, pl


def test_walk_and_overflow_decode(world):
    """d. n = 2 * stride * 64 + 1: wave 0 walks chunks 0, stride and 2 * stride (one frame); the chunks of a wave differ
    lane by lane in alignment and content; 40 + 40, 64 + 1 and 64 + 64 long headers in three waves' first two chunks (and 20 + 20, which
    does not overflow)."""
    case, pl = _walk(world)
    report("walk", pl, n=case.n, waves_with_3_chunks=int(sum(len(pl.wave_chunks(w)) >= 3 for w in range(pl.n_waves))),
           min_deferred_by_overflow=int(pl.min_deferred.sum()))
    t0 = time.perf_counter()
    check_decode(world, case)
    print("walk n=%d: decode checked in %.2f s" % (case.n, time.perf_counter() - t0))


def test_walk_and_overflow_stamp(world):
    """d, stamping: the size pass and the write pass must make the same held / deferred split."""
    case, _ = _walk(world)
    t0 = time.perf_counter()
    check_stamp(world, case)
    print("walk n=%d: stamp checked in %.2f s" % (case.n, time.perf_counter() - t0))


def test_threshold_and_tiny_buffer(world):
    """e. The same buffer at n = 65,535 (simple) and n = 65,536 (pipelined) gives identical results; nbytes = 7 with
    n = 65,536 takes the simple form and every frame is MALFORMED."""
    case = world.case("bounds", lambda: R.case_bounds(world.cus))
    n = R.K_PIPE_MIN_FRAMES
    assert case.n == n and case.plan(world.cus, n).pipelined and not case.plan(world.cus, n - 1).pipelined
    (d0, s0), (d1, s1) = check_both(world, case, n - 1), check_both(world, case, n)
    for so in d0:
        np.testing.assert_array_equal(d0[so][0], d1[so][0][:n - 1])
        np.testing.assert_array_equal(d0[so][1].view(np.uint8), d1[so][1][:n - 1].view(np.uint8))
    np.testing.assert_array_equal(s0[0], s1[0][:n - 1])
    assert not R.launch_shape(n, 7, world.cus)[0]
    for so in (L.SENDER_FROM_HEADER, 3):
        st, rec, n_bad = world.decode(case, n, so, nbytes=7)
        assert (st == L.DEC_MALFORMED).all() and not rec.view(np.uint8).any() and n_bad == n
    st, off, tot, out = world.stamp(case, n, 1024, 1024, nbytes=7)
    assert (st == L.STAMP_MALFORMED).all() and not off.any() and tot == 0 and (out == SENT).all()


@pytest.mark.parametrize("mod", range(4))
def test_buffer_end(world, mod):
    """f. nbytes % 4 = mod with the last frame ending exactly at nbytes; the last 64 frames inside the final 256 bytes
    (clamped window loads); offsets nbytes - 8 (hl = bl = 0), nbytes - 7, nbytes, nbytes + 1 and 2**33; a body that runs
    one byte past the buffer."""
    case = world.case("end%d" % mod, lambda: R.case_end(world.cus, mod))
    p, pl = case.pack(), case.plan(world.cus)
    last = p.offs[-64:].astype(np.int64).tolist()
    assert pl.pipelined and p.nbytes % 4 == mod and pl.n % 64 == 0 and min(last) >= p.nbytes - 256
    assert all(o in last for o in (p.nbytes - 8, p.nbytes - 7, p.nbytes, p.nbytes + 1, 2 ** 33))
    ends = p.offs.astype(np.int64) + 8 + p.hls + p.bls
    assert ((ends[-64:] == p.nbytes) & (pl.cls[-64:] >= R.WINDOW)).sum() >= 3
    assert ((ends[-64:] == p.nbytes + 1) & (pl.cls[-64:] == R.BAD_LENGTHS)).any()
    report(case.name, pl, nbytes=p.nbytes, last_chunk={R.CLASS_NAMES[k]: int((pl.cls[-64:] == k).sum()) for k in range(6)})
    check_both(world, case)


def test_neighbour_bytes_short(world):
    """g. Every cut (6..119) of one valid 120-byte header, the body being the rest of it, packed with no gap at all four
    alignments: MALFORMED from an LDS row (which holds the rest of the header) as from HBM."""
    case = world.case("neighbour_short", R.case_neighbour_short)
    pl = case.plan(world.cus)
    assert pl.pipelined and (pl.cls == R.WINDOW).all()
    assert (case.expect_decode()[0] == L.DEC_MALFORMED).all()
    report("neighbour_short", pl)
    check_both(world, case)
    small = world.case("neighbour_short_simple", lambda: R.case_neighbour_short(912))
    assert not small.plan(world.cus).pipelined
    check_both(world, small)


def test_neighbour_bytes_long(world):
    """g. The same with long headers cut past byte 256 (held rows) and past byte 1,040 (big[])."""
    case = world.case("neighbour_long", lambda: R.case_neighbour_long(world.cus))
    p, pl = case.pack(), case.plan(world.cus)
    assert pl.pipelined and len(pl.overflowing) == 0
    held = pl.surely_held & (p.hls + p.bls == R.CUT_HELD_LEN) & (p.hls >= R.CUT_HELD_FROM)
    big = (pl.cls == R.TOO_LONG_LDS) & (p.hls + p.bls == R.CUT_BIG_LEN) & (p.hls >= R.CUT_BIG_FROM)
    for q in range(4):
        at = (p.offs & np.uint64(3)) == q
        assert set(p.hls[held & at].tolist()) == set(range(R.CUT_HELD_FROM, R.CUT_HELD_LEN)), q
        assert set(p.hls[big & at].tolist()) == set(range(R.CUT_BIG_FROM, R.CUT_BIG_LEN)), q
    assert (case.expect_decode()[0][held | big] == L.DEC_MALFORMED).all()
    report("neighbour_long", pl, held_cuts=int(held.sum()), big_cuts=int(big.sum()))
    check_both(world, case)
    small = world.case("neighbour_long_simple", lambda: R.specials_only("neighbour_long_simple", R.neighbour_long_specials()))
    assert not small.plan(world.cus).pipelined
    check_both(world, small)
