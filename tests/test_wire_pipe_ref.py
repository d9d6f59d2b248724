"""tests/wire_pipe_ref.py held to the kernel text, to the oracle and to its own claims, without a GPU: the constants and
boundary expressions it restates are the ones in orleans_amd/csrc/wire_codec.hip; the memoised expectations equal the
oracle run over the whole packed buffer; and for 8, 64, 256 and 304 CUs the case lists reach every path class, every
boundary at every alignment, every held-batch size, an overflowing wave and a three-chunk walk with a partial last chunk.
This test fails when a case list stops reaching a regime."""
import os
import re

import numpy as np
import pytest

import wire_corpus as C
import wire_pipe_ref as R
from oracle import wire_codec as W
from oracle.pyref import Key

_CASES = {}   # the case lists for one CU count, built once
SRC = os.path.join(os.path.dirname(__file__), "..", "orleans_amd", "csrc", "wire_codec.hip")


def _src():
    with open(SRC, encoding="utf-8") as f:
        return f.read()


def _constexpr(src, name, known):
    m = re.search(r"^constexpr\s+(?:uint32_t|size_t)\s+%s\s*=\s*([^;]+);" % name, src, re.M)
    assert m, name
    return eval(re.sub(r"(\d)u\b", r"\1", m.group(1)), {"__builtins__": {}}, dict(known))


def test_constants_match_the_kernel_text():
    src = _src()
    k = {}
    for name in ("kRowWords", "kRowStride", "kHeldWords", "kHeldMax", "kLongWords", "kPipeMinFrames"):
        k[name] = _constexpr(src, name, k)
    assert k["kRowStride"] == k["kRowWords"] + 1
    assert (k["kRowWords"], k["kHeldWords"], k["kHeldMax"], k["kLongWords"], k["kPipeMinFrames"]) == (
        R.K_ROW_WORDS, R.K_HELD_WORDS, R.K_HELD_MAX, R.K_LONG_WORDS, R.K_PIPE_MIN_FRAMES)
    flat = re.sub(r"\s+", " ", src)
    # the window rule, in the decoder (fits) and in both stamp passes (does not fit)
    assert flat.count("(uint64_t)hl <= kRowWords * 4 - 8 - q0") == 1
    assert flat.count("(uint64_t)hl > kRowWords * 4 - 8 - q0") == 1
    # the held-row rule, over fw = words from the frame's first aligned word to its header's last byte
    assert flat.count("const uint32_t fw = (uint32_t)(((foff & 3u) + 8u + (uint64_t)fhl + 3u) / 4u);") == 2
    assert flat.count("if (nw > kHeldWords) continue;") == 2
    assert flat.count("if (fw <= kHeldWords)") == 2
    assert flat.count("if (k < kHeldMax)") == 2
    assert flat.count("min(n_held[wv], kHeldMax)") == 2
    # the LDS / HBM rule of the deferred decoder
    assert flat.count("const uint32_t words = (uint32_t)(((off & 3u) + 8u + (uint64_t)hl + 3u) / 4u);") == 1
    assert flat.count("if (nw <= kLongWords)") == 2
    # the launchers
    assert flat.count("n >= kPipeMinFrames && nbytes >= 8") == 2
    assert "std::min<uint32_t>((uint32_t)cus * 2u, (chunks + 3) / 4)" in flat
    assert "std::min<uint32_t>((uint32_t)cus * 2u, (uint32_t)(((n + 63) / 64 + 3) / 4))" in flat
    assert flat.count("const uint32_t stride = gridDim.x * 4;") == 2
    assert flat.count("uint32_t c = blockIdx.x * 4 + wv;") == 2


def test_launch_shape():
    assert R.launch_shape(65535, 1 << 20, 256) == (False, 256, 0, 1024)
    assert R.launch_shape(65536, 7, 256)[0] is False
    assert R.launch_shape(65536, 8, 256) == (True, 256, 1024, 1024)
    assert R.launch_shape(72360, 1 << 20, 256) == (True, 283, 1132, 1131)   # the existing decode test: one chunk per wave
    assert R.launch_shape(262145, 1 << 20, 256) == (True, 512, 2048, 4097)
    p = R.plan(262145, 1 << 30, np.arange(262145) * 100, np.full(262145, 80), 256)
    assert p.wave_chunks(0) == [0, 2048, 4096] and p.wave_chunks(1) == [1, 2049] and p.n_waves == 2048
    assert R.walk_n(256) == 262145 and R.walk_n(8) >= R.K_PIPE_MIN_FRAMES


def test_classes_at_their_boundaries():
    nb = 1 << 20
    for q in range(4):
        for hl, want in ((248 - q, R.WINDOW), (249 - q, R.HELD_FITS), (1032 - q, R.HELD_FITS), (1033 - q, R.TOO_LONG_LDS),
                         (4088 - q, R.TOO_LONG_LDS), (4089 - q, R.TOO_LONG_HBM)):
            assert R.classify(nb, [400 + q], [hl], [0])[0] == want, (q, hl)
            assert R.window_fits(q, hl) == (want == R.WINDOW)
    assert R.classify(100, [92, 93, 100, 101, 2 ** 33], [0] * 5, [0] * 5).tolist() == [R.WINDOW] + [R.BAD_PREFIX] * 4
    assert R.classify(100, [0, 0, 0, 0], [-1, 0, 92, 93], [0, -1, 0, 0]).tolist() == [R.BAD_LENGTHS, R.BAD_LENGTHS, R.WINDOW,
                                                                                       R.BAD_LENGTHS]


@pytest.mark.parametrize("L", list(range(245, 250)) + list(range(1027, 1034)) + list(range(4083, 4090)) + [73, 20000])
def test_exact_length_headers_decode(L):
    for gl in (False, True):
        h = R.routing_header(L, gl, gid=L, seed=L % 50)
        assert len(h) == L
        d = W.decode_for_route(h, C.silo_index())
        assert d.status == W.DEC_OK and d.n1 == L
        if gl:   # the header's last 30 bytes are the TARGET_GRAIN entry
            assert h[-30] == W.H_TARGET_GRAIN
    with pytest.raises(AssertionError):
        R.routing_header(72)


def test_neighbour_cuts_are_all_malformed():
    for e in R.case_neighbour_short().entries + [e for e, _ in R.neighbour_long_specials()]:
        hl, bl = np.frombuffer(e.frame[:8], "<i4")
        assert 8 + hl + bl == len(e.frame)
        assert W.decode_for_route(e.frame[8:8 + hl], C.silo_index()).status == W.DEC_MALFORMED
        assert W.decode_for_route(e.frame[8:], C.silo_index()).status == W.DEC_OK   # the whole header is valid
    assert len(R.case_neighbour_short().entries) == 2 * 114


def test_stamp_forms_have_their_statuses():
    for g, L in enumerate(R.STAMP_LENGTHS):
        forms = R.stamp_forms(L, 0, g)
        assert {f[2] for f in forms} == set(R.STAMP_FORM_STATUS)
        for e, _, name in forms:
            st, out = R.MEMO.stamp(e)
            assert st == R.STAMP_FORM_STATUS[name], (L, name, st)
            if name == "new_registered_reuse":   # both PRIOR_MESSAGE slots reused: activation, then silo, in their places
                keys = [k for k, _ in _items(out)]
                i = keys.index(W.H_TARGET_SILO)
                assert keys[i:i + 2] == [W.H_TARGET_SILO, W.H_TARGET_ACTIVATION]
                assert keys[-2:] == [W.H_IS_NEW_PLACEMENT, W.H_NEW_GRAIN_TYPE]
            if name == "hit_changed":
                keys = [k for k, _ in _items(out)]
                assert W.H_PRIOR_MESSAGE_ID not in keys and W.H_PRIOR_MESSAGE_TIMES not in keys and W.H_TARGET_SILO in keys
            if name == "hit_same":
                assert W.H_PRIOR_MESSAGE_ID in [k for k, _ in _items(out)]


def _items(frame):
    hl = int.from_bytes(frame[:4], "little")
    return list(W.parse_headers(frame[8:8 + hl]).items())


@pytest.mark.parametrize("name", ["window", "bounds", "batches", "walk", "end0", "end1", "end2", "end3", "neighbour_short",
                                  "neighbour_long"])
def test_memoised_expectation_equals_the_oracle_on_the_buffer(name):
    if not _CASES:
        _CASES.update({c.name: c for c in R.all_cases(64)})
    case = _CASES[name].cut(5000)
    assert case.n <= 5000
    p = case.pack()
    offs = [int(o) for o in p.offs]
    for so in (W.SENDER_FROM_HEADER, 3):
        st, rec, n_bad = case.expect_decode(so)
        st_ref, rec_ref = C.oracle_decode(p.buf, p.nbytes, p.offs, so)
        np.testing.assert_array_equal(st, st_ref)
        np.testing.assert_array_equal(rec.view(np.uint8), rec_ref.view(np.uint8))
        assert n_bad == int((st_ref != 0).sum())
    nk = [Key(int(x[0]), int(x[1]), int(x[2]), None) for x in p.new_keys]
    ref = W.stamp_frames(bytes(p.buf[:p.nbytes]), offs, p.route, p.act, R.ACT_KEYS, nk, R.SILO_OF, R.GRAIN_TYPES)
    st, sizes, ooff, total, exp, msk = case.expect_stamp()
    np.testing.assert_array_equal(st, np.array([s for s, _ in ref], np.uint8))
    assert sizes.tolist() == [(len(b) + 3) // 4 * 4 for _, b in ref] and total == int(sizes.sum())
    for i, (_, b) in enumerate(ref):
        o = int(ooff[i])
        assert bytes(exp[o:o + len(b)]) == b and msk[o:o + len(b)].all() and not msk[o + len(b):o + int(sizes[i])].any(), i
    # the packing gave every frame the alignment it asked for, with the fewest zero bytes
    nb = case.n_body
    assert ((p.offs[:nb] & np.uint64(3)) == case.q0).all()
    ends = p.offs[:nb].astype(np.int64) + 8 + p.hls[:nb] + p.bls[:nb]
    assert (p.offs[1:nb].astype(np.int64) - ends[:-1] < 4).all() and (p.offs[1:nb].astype(np.int64) >= ends[:-1]).all()


@pytest.mark.parametrize("cus", R.CUS_LIST)
def test_reach(cus):
    calls0 = R.MEMO.calls
    seen = np.zeros(6, np.int64)

    # a. the window boundary, pipelined and on a 300-frame prefix
    case = R.case_window(cus)
    p = case.pack()
    for n in (R.N_PIPE, 300):
        pl = case.plan(cus, n)
        assert pl.pipelined == (n == R.N_PIPE)
        s = (p.offs[:n] & np.uint64(3)).astype(np.int64) + 8 + p.hls[:n]
        for q in range(4):
            at = (p.offs[:n] & np.uint64(3)) == q
            for tot, want in ((255, R.WINDOW), (256, R.WINDOW), (257, R.HELD_FITS)):
                hit = at & (s == tot)
                assert hit.sum() >= 2 and (pl.cls[hit] == want).all(), (n, q, tot)
                if n == R.N_PIPE and tot == 257:
                    assert (hit & pl.surely_held).any(), (q, "held whatever the atomics' order")
    seen += np.bincount(case.plan(cus).cls, minlength=6)

    # b. the held-row and big[] boundaries, the 20,000-byte header, the stamp statuses at held and deferred lengths
    case = R.case_bounds(cus)
    p, pl = case.pack(), case.plan(cus)
    assert pl.pipelined and len(pl.overflowing) == 0
    s = (p.offs & np.uint64(3)).astype(np.int64) + 8 + p.hls
    fw = R.frame_words(p.offs.astype(np.int64) & 3, p.hls)
    for q in range(4):
        at = (p.offs & np.uint64(3)) == q
        for tot, words, want in zip(R.BOUND_SUMS, (259, 260, 260, 261, 1023, 1024, 1024, 1025),
                                    (R.HELD_FITS,) * 3 + (R.TOO_LONG_LDS,) * 4 + (R.TOO_LONG_HBM,)):
            hit = at & (s == tot)
            assert hit.sum() >= 2 and (fw[hit] == words).all() and (pl.cls[hit] == want).all(), (q, tot)
    assert (p.hls == R.HUGE).any()
    st = case.expect_stamp()[0]
    for L, want in zip(R.STAMP_LENGTHS, (R.HELD_FITS, R.TOO_LONG_LDS, R.TOO_LONG_HBM)):
        hit = p.hls == L
        assert (pl.cls[hit] == want).all()
        assert set(st[hit].tolist()) == {W.STAMP_OK, W.STAMP_COMPLETE, W.STAMP_SKIPPED, W.STAMP_UNSUPPORTED, W.STAMP_MALFORMED}
        assert len(set(case.eidx[hit].tolist())) == len(R.STAMP_FORM_STATUS)
    seen += np.bincount(pl.cls, minlength=6)

    # c. held batches: every count, one long-bearing chunk per wave, long frames at the first and last lanes
    case = R.case_batches(cus)
    p, pl = case.pack(), case.plan(cus)
    assert pl.pipelined and len(pl.overflowing) == 0 and set(np.unique(pl.cls).tolist()) == {R.WINDOW, R.HELD_FITS}
    assert set(R.HELD_COUNTS) <= set(pl.wave_long[:pl.n_waves].tolist())
    if cus == 256:
        assert pl.stride >= pl.n_chunks   # one chunk per wave
    for w in range(pl.n_waves):
        assert sum(pl.chunk_long[c] > 0 for c in pl.wave_chunks(w)) <= 1
    for c in range(min(pl.n_waves, 9)):
        lanes = np.nonzero(pl.long[c * 64:(c + 1) * 64])[0].tolist()
        assert lanes == sorted(R.spread_lanes(R.HELD_COUNTS[c])), c
        ids = list(zip(case.eidx[c * 64:(c + 1) * 64][lanes].tolist(), case.q0[c * 64:(c + 1) * 64][lanes].tolist()))
        # rows k and k + 1, and the rows that share a slot in consecutive batches (k and k + 16), hold different frames
        for d in (1, 16):
            for a, b in zip(ids, ids[d:]):
                ea, eb = case.entries[a[0]], case.entries[b[0]]
                assert ea.frame != eb.frame and len(ea.frame) != len(eb.frame), (c, d)
        assert len(lanes) < 4 or len({q for _, q in ids}) == 4

    # d. the walk: three chunks (or more on a small device) with a partial last chunk, differing lane by lane; overflow
    case = R.case_walk(cus)
    p, pl = case.pack(), case.plan(cus)
    assert pl.pipelined and pl.stride == 8 * cus and pl.blocks == 2 * cus
    ch = pl.wave_chunks(0)
    assert len(ch) >= 3 and (len(ch) == 3 or cus < 64) and pl.n - ch[-1] * 64 == 1
    assert cus != 256 or pl.n == 262145
    for w in (0, 1, 2, pl.stride - 1):   # waves of short frames only
        ch = pl.wave_chunks(w)
        for a, b in ((0, 1), (1, 2), (0, 2)):
            if b >= len(ch):
                continue
            m = min(64, pl.n - ch[b] * 64)
            ia, ib = ch[a] * 64 + np.arange(m), ch[b] * 64 + np.arange(m)
            assert ((p.offs[ia] & np.uint64(3)) != (p.offs[ib] & np.uint64(3))).all(), (w, a, b)
            assert (case.eidx[ia] != case.eidx[ib]).all(), (w, a, b)
    for w, (c0, c1) in R.WALK_WAVES.items():
        assert [int(pl.chunk_long[c]) for c in pl.wave_chunks(w)[:2]] == [c0, c1]
        assert pl.wave_long[w] == c0 + c1 and pl.min_deferred[w] == max(c0 + c1 - 64, 0)
        sel = np.zeros(pl.n, bool)
        for c in pl.wave_chunks(w)[:2]:
            sel[c * 64:(c + 1) * 64] = True
        assert (pl.cls[sel & pl.long] == R.HELD_FITS).any() and (pl.cls[sel & pl.long] >= R.TOO_LONG_LDS).any()
    assert pl.overflowing.tolist() == R.WALK_OVERFLOWING == [5, 9, 13] and pl.surely_held.sum() >= 20
    assert (pl.cls == R.TOO_LONG_HBM).any()
    seen += np.bincount(pl.cls, minlength=6)

    # f. the buffer's end
    for mod in range(4):
        case = R.case_end(cus, mod)
        p, pl = case.pack(), case.plan(cus)
        assert pl.pipelined and p.nbytes % 4 == mod and pl.n % 64 == 0
        last = p.offs[-64:].astype(np.int64)
        assert (last >= p.nbytes - 256).all()
        for want in (p.nbytes - 8, p.nbytes - 7, p.nbytes, p.nbytes + 1, 2 ** 33):
            assert want in last.tolist()
        i = last.tolist().index(p.nbytes - 8) + pl.n - 64
        assert p.hls[i] == 0 and p.bls[i] == 0 and pl.cls[i] == R.WINDOW
        ends = p.offs.astype(np.int64) + 8 + p.hls + p.bls
        ok = pl.cls >= R.WINDOW
        assert (ends[-64:][ok[-64:]] == p.nbytes).sum() >= 3       # frames that end exactly at nbytes
        assert (ends[-64:][pl.cls[-64:] == R.BAD_LENGTHS] == p.nbytes + 1).any()   # a body one byte past the buffer
        assert (pl.cls[-64:] == R.BAD_PREFIX).sum() >= 4
        seen += np.bincount(pl.cls, minlength=6)

    # g. neighbour bytes
    case = R.case_neighbour_short()
    p, pl = case.pack(), case.plan(cus)
    assert pl.pipelined and (pl.cls == R.WINDOW).all()
    assert (np.diff(p.offs.astype(np.int64)) == 128).sum() == pl.n - 4   # no gap inside a region
    for q in range(4):
        assert len(set(case.eidx[(p.offs & np.uint64(3)) == q].tolist())) == 228
    small = R.case_neighbour_short(912)
    assert not small.plan(cus).pipelined and all(
        len(set(small.eidx[(small.pack().offs & np.uint64(3)) == q].tolist())) == 228 for q in range(4))
    case = R.case_neighbour_long(cus)
    p, pl = case.pack(), case.plan(cus)
    assert pl.pipelined and len(pl.overflowing) == 0
    n_sp = len(R.neighbour_long_specials())
    held = pl.surely_held & (p.hls >= R.CUT_HELD_FROM) & (p.hls < R.CUT_HELD_LEN) & (p.hls + p.bls == R.CUT_HELD_LEN)
    big = (pl.cls == R.TOO_LONG_LDS) & (p.hls >= R.CUT_BIG_FROM) & (p.hls + p.bls == R.CUT_BIG_LEN)
    for q in range(4):
        at = (p.offs & np.uint64(3)) == q
        assert set(p.hls[held & at].tolist()) == set(range(R.CUT_HELD_FROM, R.CUT_HELD_LEN)), q
        assert set(p.hls[big & at].tolist()) == set(range(R.CUT_BIG_FROM, R.CUT_BIG_LEN)), q
    simple = R.specials_only("neighbour_long_simple", R.neighbour_long_specials())
    assert simple.n == n_sp and not simple.plan(cus).pipelined

    assert (seen > 0).all(), dict(zip(R.CLASS_NAMES, seen.tolist()))   # every path class
    # a few hundred oracle calls per case, whatever n is
    assert R.MEMO.calls - calls0 < 3000
