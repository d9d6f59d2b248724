"""The wire codec's launch plan restated, frame builders of exact length, memoised oracle expectations and the case
lists of tests/test_gpu_wire_pipe.py (test infrastructure, CPU only; tests/test_wire_pipe_ref.py asserts, without a GPU,
which regimes the case lists reach).

The plan restates launch_decode_frames / launch_stamp_frames and the two pipelined kernels of
orleans_amd/csrc/wire_codec.hip: which form runs, how many workgroups, which 64-frame chunks each persistent wave walks,
and for every frame which path parses it:

  bad_prefix     the 8 length bytes are not inside the buffer;
  bad_lengths    a negative length, or header + body past the buffer;
  window         the header fits the 256-byte window staged in the frame's LDS row: hl <= 256 - 8 - q0;
  held_fits      a longer header of at most kHeldWords words (counted from the frame's first aligned word): parsed
                 from a held row after the wave's last chunk, if the wave holds at most kHeldMax long headers;
  too_long_lds   more than kHeldWords words and at most kLongWords: always deferred, parsed from big[] in LDS;
  too_long_hbm   more than kLongWords words: always deferred, parsed from HBM.

A wave whose share holds more than kHeldMax long headers (of the three long classes together) overflows: which 64 it
holds is decided by the order of LDS atomics, which the plan does not predict; it reports only that at least
count - 64 of them are deferred.  Outputs must not depend on the split.

The expectations are not the plan's: they are oracle/wire_codec.py's, computed once per distinct frame (decode) or per
distinct (frame, route, activation, new key) entry (stamp) and expanded by index.  That is valid only for frames that
stand alone (8 + hl + bl == len(frame)) and lie inside the buffer; a case's tail (garbage lengths, offsets at and past
the buffer's end, overlapping frames) goes through decode_frames / stamp_frames on the real buffer.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import wire_corpus as C
from oracle import wire_codec as W
from oracle.pyref import Key, key_from_long

# orleans_amd/csrc/wire_codec.hip (tests/test_wire_pipe_ref.py pins these against its text)
K_ROW_WORDS = 64
K_HELD_WORDS = 260
K_HELD_MAX = 64
K_LONG_WORDS = 1024
K_PIPE_MIN_FRAMES = 1 << 16

BAD_PREFIX, BAD_LENGTHS, WINDOW, HELD_FITS, TOO_LONG_LDS, TOO_LONG_HBM = range(6)
CLASS_NAMES = ("bad_prefix", "bad_lengths", "window", "held_fits", "too_long_lds", "too_long_hbm")

CUS_LIST = (8, 64, 256, 304)
HELD_COUNTS = (0, 1, 15, 16, 17, 32, 33, 63, 64)


def window_fits(q0: int, hl: int) -> bool:
    return hl <= K_ROW_WORDS * 4 - 8 - q0


def frame_words(q0, hl):
    """Words from the frame's first aligned word to the word of its header's last byte (fw / nw in the kernels)."""
    return (q0 + 8 + hl + 3) // 4


# ---------------------------------------------------------------------------------------------------------------------
# the launch plan
# ---------------------------------------------------------------------------------------------------------------------
def launch_shape(n: int, nbytes: int, cus: int) -> Tuple[bool, int, int, int]:
    """(pipelined, blocks, stride in chunks, n_chunks) of launch_decode_frames / launch_stamp_frames."""
    n_chunks = (n + 63) // 64
    pipelined = n >= K_PIPE_MIN_FRAMES and nbytes >= 8
    if not pipelined:
        return False, (n + 255) // 256, 0, n_chunks
    blocks = min(2 * cus, (n_chunks + 3) // 4)
    return True, blocks, 4 * blocks, n_chunks


def read_lengths(buf: np.ndarray, nbytes: int, offs) -> Tuple[np.ndarray, np.ndarray]:
    """The two int32 lengths at every offset whose 8 prefix bytes lie inside the buffer (0 elsewhere)."""
    o = np.asarray(offs).astype(np.int64)
    ok = (o >= 0) & (o <= nbytes) & (nbytes - o >= 8)
    at = np.where(ok, o, 0)[:, None] + np.arange(8)
    b = np.ascontiguousarray(buf[:max(nbytes, 8)][at].astype(np.uint8)).view("<i4").astype(np.int64)
    return np.where(ok, b[:, 0], 0), np.where(ok, b[:, 1], 0)


def classify(nbytes: int, offs, hls, bls) -> np.ndarray:
    o = np.asarray(offs).astype(np.int64)  # every offset the tests use is below 2**63
    hls = np.asarray(hls, np.int64)
    bls = np.asarray(bls, np.int64)
    ok_prefix = (o >= 0) & (o <= nbytes) & (nbytes - o >= 8)
    ok_len = (hls >= 0) & (bls >= 0) & (hls + bls <= nbytes - o - 8)
    q0 = o & 3
    fw = frame_words(q0, hls)
    cls = np.full(len(o), WINDOW, np.uint8)
    cls[hls > K_ROW_WORDS * 4 - 8 - q0] = HELD_FITS
    cls[fw > K_HELD_WORDS] = TOO_LONG_LDS
    cls[fw > K_LONG_WORDS] = TOO_LONG_HBM
    cls[~ok_len] = BAD_LENGTHS
    cls[~ok_prefix] = BAD_PREFIX
    return cls


@dataclass
class Plan:
    n: int
    pipelined: bool
    blocks: int
    stride: int             # chunks between two chunks of one wave (0 in the simple form)
    n_chunks: int
    cls: np.ndarray         # path class per frame
    chunk_long: np.ndarray  # long headers per chunk
    wave_long: np.ndarray   # long headers per wave's share (pipelined form; wave w walks chunks w, w + stride, ...)

    def wave_chunks(self, w: int) -> List[int]:
        return list(range(w, self.n_chunks, self.stride)) if self.pipelined else []

    def wave_of(self, i):
        return (np.asarray(i) // 64) % self.stride

    @property
    def n_waves(self) -> int:
        return min(self.stride, self.n_chunks) if self.pipelined else 0

    @property
    def overflowing(self) -> np.ndarray:
        """Waves whose share holds more than kHeldMax long headers."""
        return np.nonzero(self.wave_long > K_HELD_MAX)[0]

    @property
    def min_deferred(self) -> np.ndarray:
        """Per wave, the least number of frames left to the deferred kernels because the held list is full."""
        return np.maximum(self.wave_long.astype(np.int64) - K_HELD_MAX, 0)

    @property
    def long(self) -> np.ndarray:
        return self.cls >= HELD_FITS

    @property
    def surely_held(self) -> np.ndarray:
        """Frames parsed from a held row whatever the atomics' order: held_fits in a wave that does not overflow."""
        if not self.pipelined:
            return np.zeros(self.n, bool)
        return (self.cls == HELD_FITS) & (self.wave_long[self.wave_of(np.arange(self.n))] <= K_HELD_MAX)

    @property
    def surely_deferred(self) -> np.ndarray:
        return (self.cls >= TOO_LONG_LDS) if self.pipelined else np.zeros(self.n, bool)

    def counts(self) -> Dict[str, int]:
        return {CLASS_NAMES[k]: int((self.cls == k).sum()) for k in range(6)}


def plan(n: int, nbytes: int, offs, hls, cus: int, bls=None) -> Plan:
    """hls / bls: the int32 lengths at each offset (read_lengths); bls defaults to 0."""
    offs = np.asarray(offs)[:n]
    hls = np.asarray(hls)[:n]
    bls = np.zeros(n, np.int64) if bls is None else np.asarray(bls)[:n]
    pipelined, blocks, stride, n_chunks = launch_shape(n, nbytes, cus)
    cls = classify(nbytes, offs, hls, bls)
    chunk = np.arange(n) // 64
    lng = cls >= HELD_FITS
    chunk_long = np.bincount(chunk[lng], minlength=n_chunks)
    wave_long = np.bincount(chunk[lng] % stride, minlength=stride) if pipelined else np.zeros(0, np.int64)
    return Plan(n, pipelined, blocks, stride, n_chunks, cls, chunk_long, wave_long)


# ---------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------
N_SILOS = C.N_SILOS
TYPE_REG, TYPE_UNREG = 4242, 4343          # a registered and an unregistered grain type code
GRAIN_TYPES = {TYPE_REG: "Grains.Registered.é"}
N_ACT_KEYS = 8
ACT_KEYS = [Key(0, 100 + i, 200 + i, None) for i in range(N_ACT_KEYS)]
NEW_KEYS = [Key(0, 900 + i, 7000 + i, None) for i in range(4)]
SILO_OF = {s: C.silo_addr(s) for s in range(N_SILOS)}
FILLER_KEY = 5
BASE_LEN, MIN_LEN = 67, 73


def route_word(status: int, host: int) -> int:
    return (status << 16) | (host << 8)


def filler_bytes(k: int, seed: int) -> bytes:
    """k printable ASCII bytes that differ from seed to seed at every position."""
    return ((np.arange(k, dtype=np.int64) * 13 + seed * 7 + (seed >> 3)) % 94 + 33).astype(np.uint8).tobytes()


def routing_header(L: int, grain_last: bool = False, gid: int = 1, seed: int = 0, silo: int = 1, tcode: int = TYPE_REG,
                   ext: Optional[str] = None, extra: Sequence[Tuple[int, tuple]] = (), bad_utf8: bool = False,
                   overrun: int = 0) -> bytes:
    """A valid routing header of exactly L bytes: category, sending silo, target grain (67 bytes), `extra`, and one
    string header that pads it (6 bytes with an empty string, so L >= 73).  The filler is the last entry, or, with
    grain_last, TARGET_GRAIN is, so that the header's final bytes carry routed data.  bad_utf8 makes the filler's last
    byte 0xFF (a string the stamp path cannot re-serialize); overrun declares the filler that many bytes longer than
    the header holds (MALFORMED at the header's far end)."""
    cat = (W.H_CATEGORY, ("int", 2))
    snd = (W.H_SENDING_SILO, ("silo", C.silo_addr(silo)))
    tg = (W.H_TARGET_GRAIN, ("grain", key_from_long(gid, tcode, ext)))
    fixed = [cat, snd, tg] + list(extra)
    k = L - len(W.serialize_headers(fixed)) - 6
    assert k >= 0, (L, k)
    fb = bytearray(filler_bytes(k, seed))
    if bad_utf8:
        assert k > 0
        fb[-1] = 0xFF
    fill = (FILLER_KEY, ("raw", bytes([W.T_STRING]) + struct.pack("<i", k + overrun) + bytes(fb)))
    items = [cat, snd] + list(extra) + [fill, tg] if grain_last else fixed + [fill]
    h = W.serialize_headers(items)
    assert len(h) == L
    return h


@dataclass(frozen=True)
class Entry:
    """One distinct frame with what the stamp call is told about it."""
    frame: bytes
    route: int = 0
    act: int = 0
    nk: int = 0   # index into NEW_KEYS


def entry(hdr: bytes, body: bytes = b"", status: int = 0, host: int = 2, act: int = 0, nk: int = 0) -> Entry:
    return Entry(W.frame(hdr, body), route_word(status, host), act, nk)


def small_entries() -> List[Entry]:
    """37 distinct short frames (all `window`): lengths 73..132, both variants, every sender, KeyExt targets, complete
    addresses, bodies of 0..6 bytes, and every route status the stamp path tells apart."""
    out = []
    statuses = [0, 1, 3, 8, 0, 1, 2]
    for j in range(37):
        extra = []
        if j % 6 == 1:
            extra = [(W.H_TARGET_SILO, ("silo", C.silo_addr(j % N_SILOS))), (W.H_TARGET_ACTIVATION, ("act", ACT_KEYS[j % 8]))]
        elif j % 6 == 4:
            extra = [(W.H_PRIOR_MESSAGE_ID, ("corr", j)), (W.H_TARGET_ACTIVATION, ("act", ACT_KEYS[3]))]
        L = MIN_LEN + len(W.serialize_headers(extra)) - 5 + (j * 5) % 60 + (8 if j % 5 == 2 else 0)
        h = routing_header(L, grain_last=bool(j & 1), gid=1000 + j, seed=j, silo=j % N_SILOS,
                           tcode=TYPE_UNREG if j % 7 == 3 else TYPE_REG, ext="k%d" % j if j % 5 == 2 else None, extra=extra)
        out.append(entry(h, bytes(range(1, 1 + j % 7)), statuses[j % 7], host=j % N_SILOS, act=j % (N_ACT_KEYS + 2), nk=j % 4))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# memoised expectations
# ---------------------------------------------------------------------------------------------------------------------
def _rec(d) -> tuple:
    return (d.tcd, d.n0, d.n1, d.sending_silo, d.category, d.flags, d.target_silo, d.aux)


def _split(frame: bytes) -> Tuple[bytes, bytes]:
    hl, bl = struct.unpack("<ii", frame[:8])
    assert hl >= 0 and bl >= 0 and 8 + hl + bl == len(frame), "memoisation needs a frame that stands alone"
    return frame[8:8 + hl], frame[8 + hl:]


class Memo:
    """The oracle's answer per distinct frame / entry, computed once."""

    def __init__(self):
        self._dec: Dict[Tuple[bytes, int], tuple] = {}
        self._stp: Dict[Entry, Tuple[int, bytes]] = {}
        self.calls = 0

    def decode(self, frame: bytes, so: int):
        k = (frame, so)
        if k not in self._dec:
            self.calls += 1
            d = W.decode_for_route(_split(frame)[0], C.silo_index(), so)
            self._dec[k] = (d.status, _rec(d))
        return self._dec[k]

    def stamp(self, e: Entry):
        if e not in self._stp:
            self.calls += 1
            hdr, body = _split(e.frame)
            ak = ACT_KEYS[e.act] if e.act < N_ACT_KEYS else None
            self._stp[e] = W.stamp_frame(hdr, body, e.route, ak, NEW_KEYS[e.nk], SILO_OF, GRAIN_TYPES)
        return self._stp[e]


MEMO = Memo()


@dataclass
class Tail:
    """Frames that do not stand alone: `data` is appended after the packed frames so that the buffer ends at
    nbytes % 4 == mod, and `offs` are resolved against it: ("tail", p) -> tail start + p, ("end", d) -> nbytes + d,
    ("abs", v) -> v.  Their expectations come from the oracle run on the real buffer."""
    data: bytes
    offs: List[Tuple[str, int]]
    mod: int = 0


@dataclass
class Packed:
    buf: np.ndarray
    nbytes: int
    offs: np.ndarray      # uint64
    route: np.ndarray     # uint32
    act: np.ndarray       # uint32
    new_keys: np.ndarray  # KEY_DTYPE-shaped (n, 3) uint64: tcd, n0, n1
    hls: np.ndarray
    bls: np.ndarray


class Case:
    """Frame i is entries[eidx[i]] starting at alignment q0[i], packed with the fewest zero bytes (0..3) that give that
    alignment; then the tail, if any."""

    def __init__(self, name: str, entries: List[Entry], eidx, q0, tail: Optional[Tail] = None):
        self.name, self.entries, self.tail = name, entries, tail
        self.eidx = np.asarray(eidx, np.int32)
        self.q0 = np.asarray(q0, np.uint8)
        assert len(self.eidx) == len(self.q0) and (self.q0 < 4).all() and self.eidx.max(initial=0) < len(entries)
        self._packed = None

    @property
    def n_body(self) -> int:
        return len(self.eidx)

    @property
    def n(self) -> int:
        return self.n_body + (len(self.tail.offs) if self.tail else 0)

    def pack(self) -> Packed:
        if self._packed is not None:
            return self._packed
        lens = [len(e.frame) for e in self.entries]
        frames = [e.frame for e in self.entries]
        zeros = [bytes(k) for k in range(4)]
        offs, pieces, pos = [], [], 0
        for e, q in zip(self.eidx.tolist(), self.q0.tolist()):
            g = (q - pos) & 3
            if g:
                pieces.append(zeros[g])
            offs.append(pos + g)
            pieces.append(frames[e])
            pos += g + lens[e]
        route = [self.entries[e].route for e in range(len(self.entries))]
        act = [self.entries[e].act for e in range(len(self.entries))]
        nk = [self.entries[e].nk for e in range(len(self.entries))]
        r = np.array(route, np.uint32)[self.eidx]
        a = np.array(act, np.uint32)[self.eidx]
        k = np.array(nk, np.int64)[self.eidx]
        if self.tail:
            t = self.tail
            g = (t.mod - len(t.data) - pos) & 3
            pieces += [zeros[g], t.data]
            start = pos + g
            pos = start + len(t.data)
            for kind, v in t.offs:
                offs.append({"tail": start + v, "end": pos + v, "abs": v}[kind])
            m = len(t.offs)
            j = np.arange(m)
            r = np.concatenate([r, np.array([route_word([0, 1, 3, 8][x % 4], x % N_SILOS) for x in range(m)], np.uint32)])
            a = np.concatenate([a, (j % N_ACT_KEYS).astype(np.uint32)])
            k = np.concatenate([k, j % 4])
        nbytes = pos
        pieces.append(bytes(-pos % 4))
        buf = np.frombuffer(b"".join(pieces), np.uint8).copy()
        if len(buf) < 8:
            buf = np.concatenate([buf, np.zeros(8 - len(buf), np.uint8)])
        nkt = np.array([[x.tcd, x.n0, x.n1] for x in NEW_KEYS], np.uint64)[k]
        o = np.array(offs, np.uint64)
        hls, bls = read_lengths(buf, nbytes, o)
        self._packed = Packed(buf, nbytes, o, r, a, nkt, hls, bls)
        return self._packed

    def plan(self, cus: int, n: Optional[int] = None) -> Plan:
        p = self.pack()
        n = self.n if n is None else n
        return plan(n, p.nbytes, p.offs, p.hls, cus, p.bls)

    def cut(self, m: int) -> "Case":
        """At most m frames of the case: up to m / 2 of its long frames and the first frames otherwise, in order, with
        the tail kept.  (Expectations are per frame, so any subset checks the expansion.)"""
        t = len(self.tail.offs) if self.tail else 0
        m = max(m - t, 0)
        if self.n_body <= m:
            return self
        p = self.pack()
        lng = np.nonzero(classify(p.nbytes, p.offs, p.hls, p.bls)[:self.n_body] >= HELD_FITS)[0][:m // 2]
        keep = np.zeros(self.n_body, bool)
        keep[lng] = True
        rest = np.nonzero(~keep)[0][:m - len(lng)]
        keep[rest] = True
        return Case(self.name + "/cut", self.entries, self.eidx[keep], self.q0[keep], self.tail)

    # -- expectations ------------------------------------------------------------------------------------------------
    def _tail_offs(self) -> List[int]:
        return [int(o) for o in self.pack().offs[self.n_body:]]

    def expect_decode(self, so: int = W.SENDER_FROM_HEADER):
        """(status u8[n], records as (n, 8) object rows -> MSG_DTYPE by the caller, n_bad)."""
        from orleans_amd import _lib as L
        per = [MEMO.decode(e.frame, so) for e in self.entries]
        st_e = np.array([s for s, _ in per], np.uint8)
        rec_e = np.zeros(len(per), L.MSG_DTYPE)
        for j, (_, r) in enumerate(per):
            rec_e[j] = r
        st, rec = st_e[self.eidx], rec_e[self.eidx]
        if self.tail:
            p = self.pack()
            dec = W.decode_frames(bytes(p.buf[:p.nbytes]), self._tail_offs(), C.silo_index(), so)
            ts = np.array([d.status for d in dec], np.uint8)
            tr = np.zeros(len(dec), L.MSG_DTYPE)
            for j, d in enumerate(dec):
                tr[j] = _rec(d)
            st, rec = np.concatenate([st, ts]), np.concatenate([rec, tr])
        return st, rec, int((st != 0).sum())

    def expect_stamp(self):
        """(status, aligned sizes, output offsets, total, expected bytes, mask of the bytes that are asserted)."""
        per = [MEMO.stamp(e) for e in self.entries]
        st = np.array([s for s, _ in per], np.uint8)[self.eidx]
        out_e = [b + bytes(-len(b) % 4) for _, b in per]
        msk_e = [b"\x01" * len(b) + bytes(-len(b) % 4) for _, b in per]
        sizes = np.array([len(b) for b in out_e], np.uint64)[self.eidx]
        ei = self.eidx.tolist()
        outs = [out_e[e] for e in ei]
        msks = [msk_e[e] for e in ei]
        if self.tail:
            p = self.pack()
            nb = self.n_body
            kd = [Key(int(x[0]), int(x[1]), int(x[2]), None) for x in p.new_keys[nb:]]
            ref = W.stamp_frames(bytes(p.buf[:p.nbytes]), self._tail_offs(), p.route[nb:], p.act[nb:], ACT_KEYS, kd, SILO_OF,
                                 GRAIN_TYPES)
            st = np.concatenate([st, np.array([s for s, _ in ref], np.uint8)])
            tb = [b + bytes(-len(b) % 4) for _, b in ref]
            sizes = np.concatenate([sizes, np.array([len(b) for b in tb], np.uint64)])
            outs += tb
            msks += [b"\x01" * len(b) + bytes(-len(b) % 4) for _, b in ref]
        offs = np.zeros(len(sizes), np.uint64)
        offs[1:] = np.cumsum(sizes)[:-1]
        exp = np.frombuffer(b"".join(outs), np.uint8)
        msk = np.frombuffer(b"".join(msks), np.uint8).astype(bool)
        return st, sizes, offs, int(sizes.sum()), exp, msk


# ---------------------------------------------------------------------------------------------------------------------
# the case lists (functions of the device's CU count)
# ---------------------------------------------------------------------------------------------------------------------
N_PIPE = K_PIPE_MIN_FRAMES


def small_pattern(n: int, stride: int, n_small: int = 37):
    """Short frames for every position: the entry and the alignment change with the lane, the chunk and the round
    (chunk // stride), so the chunks one wave walks differ lane by lane."""
    i = np.arange(n)
    lane, chunk = i % 64, i // 64
    rnd = chunk // max(stride, 1)
    return (lane * 3 + chunk + 7 * rnd) % n_small, (lane + chunk + rnd) % 4


def spread_lanes(m: int) -> List[int]:
    """m lanes of a chunk: the first ceil(m / 2) and the last floor(m / 2)."""
    return list(range((m + 1) // 2)) + list(range(64 - m // 2, 64))


def _mixed(name: str, n: int, cus: int, specials: List[Tuple[Entry, int]], per_chunk: int, tail: Optional[Tail] = None) -> Case:
    """Short frames everywhere; the specials (entry, q0), repeated in order, at per_chunk lanes (first and last lanes
    first) of each of the first min(stride, full chunks) chunks, so that every wave's share holds at most per_chunk
    of them whatever the CU count."""
    smalls = small_entries()
    _, _, stride, _ = launch_shape(n, 8, cus)
    stride = stride or (n + 63) // 64
    eidx, q0 = small_pattern(n, stride)
    uniq: Dict[Entry, int] = {}
    entries = list(smalls)
    for e, _ in specials:
        if e not in uniq:
            uniq[e] = len(entries)
            entries.append(e)
    lanes = spread_lanes(per_chunk)
    k = 0
    for c in range(min(stride, n // 64)):
        for ln in lanes:
            e, q = specials[k % len(specials)]
            eidx[c * 64 + ln], q0[c * 64 + ln] = uniq[e], q
            k += 1
    assert k >= len(specials), (name, k, len(specials))
    return Case(name, entries, eidx, q0, tail)


# a. the window boundary: q0 + 8 + hl in {255, 256, 257} at every q0, both variants
def window_specials() -> List[Tuple[Entry, int]]:
    out = []
    for q in range(4):
        for s in (255, 256, 257):
            for gl in (False, True):
                hl = s - 8 - q
                j = len(out)
                out.append((entry(routing_header(hl, gl, gid=2000 + j, seed=j, silo=j % N_SILOS), bytes([j, j + 1][:j % 3]),
                                  status=j % 2, host=j % N_SILOS, act=j % N_ACT_KEYS, nk=j % 4), q))
    return out


def case_window(cus: int, n: int = N_PIPE) -> Case:
    return _mixed("window", n, cus, window_specials(), per_chunk=12)


# b. the held-row and big[] boundaries, a 20,000-byte header, every stamp status at held and deferred lengths
BOUND_SUMS = (4 * K_HELD_WORDS - 4, 4 * K_HELD_WORDS - 3, 4 * K_HELD_WORDS, 4 * K_HELD_WORDS + 1,      # fw 259 260 260 261
              4 * K_LONG_WORDS - 4, 4 * K_LONG_WORDS - 3, 4 * K_LONG_WORDS, 4 * K_LONG_WORDS + 1)      # nw 1023 1024 1024 1025
STAMP_LENGTHS = (700, 1500, 4200)  # held, deferred through big[], deferred from HBM
HUGE = 20000


def stamp_forms(L: int, q: int, g: int) -> List[Tuple[Entry, int, str]]:
    """Every stamp status on a header of L bytes: (entry, q0, the form's name)."""
    pid, ptm = (W.H_PRIOR_MESSAGE_ID, ("corr", 77 + g)), (W.H_PRIOR_MESSAGE_TIMES, ("int", 2))
    ta = (W.H_TARGET_ACTIVATION, ("act", ACT_KEYS[3]))
    H = lambda gl=True, **kw: routing_header(L, gl, gid=3000 + g, seed=g, silo=g % N_SILOS, **kw)  # noqa: E731
    body = bytes(range(7, 7 + g % 5))
    return [
        (entry(H(extra=[pid, ta, ptm]), body, 0, host=2, act=4), q, "hit_changed"),
        (entry(H(extra=[pid, ta, ptm]), body, 0, host=2, act=3), q, "hit_same"),
        (entry(H(extra=[pid, ptm]), body, 1, host=5, nk=1), q, "new_registered_reuse"),
        (entry(H(gl=False), body, 1, host=6, nk=2), q, "new_registered"),
        (entry(H(tcode=TYPE_UNREG), body, 1, host=5, nk=1), q, "new_unregistered"),
        (entry(H(extra=[ta, (W.H_TARGET_SILO, ("silo", C.silo_addr(4)))]), body, 3, host=4), q, "complete"),
        (entry(H(), body, 8, host=1), q, "skipped"),
        (entry(H(bad_utf8=True), body, 0, host=1, act=1), q, "noncanonical"),
        (entry(H(gl=False, overrun=1), body, 0, host=1, act=1), q, "malformed_far_end"),
        (entry(H(extra=[(W.H_TARGET_ACTIVATION, ("null",))]), body, 0, host=1, act=1), q, "malformed_null_activation"),
    ]


STAMP_FORM_STATUS = {"hit_changed": W.STAMP_OK, "hit_same": W.STAMP_OK, "new_registered_reuse": W.STAMP_OK,
                     "new_registered": W.STAMP_OK, "new_unregistered": W.STAMP_UNSUPPORTED, "complete": W.STAMP_COMPLETE,
                     "skipped": W.STAMP_SKIPPED, "noncanonical": W.STAMP_UNSUPPORTED, "malformed_far_end": W.STAMP_MALFORMED,
                     "malformed_null_activation": W.STAMP_MALFORMED}


def bounds_specials() -> List[Tuple[Entry, int]]:
    out = []
    for s in BOUND_SUMS:
        for q in range(4):
            for gl in (False, True):
                j = len(out)
                out.append((entry(routing_header(s - 8 - q, gl, gid=2500 + j, seed=j, silo=j % N_SILOS), bytes(j % 4),
                                  status=j % 2, host=j % N_SILOS, act=j % N_ACT_KEYS, nk=j % 4), q))
    out.append((entry(routing_header(HUGE, True, gid=2499, seed=5), b"xy", 0, host=3, act=2), 1))
    for g, L in enumerate(STAMP_LENGTHS):
        for f in stamp_forms(L, (g + 1) % 4, g):
            out.append(f[:2])
    return out


def case_bounds(cus: int, n: int = N_PIPE) -> Case:
    return _mixed("bounds", n, cus, bounds_specials(), per_chunk=12)


# c. held batches: chunks with exactly 0, 1, 15, 16, 17, 32, 33, 63, 64 long headers, one such chunk per wave
def long_entries(n_long: int = 23, lo: int = 250, hi: int = 1029, base_gid: int = 4000) -> List[Entry]:
    """Distinct long frames, hl spread over [lo, hi]: neighbours differ in length, variant, sender, target and body."""
    out = []
    for j in range(n_long):
        hl = lo + (hi - lo) * ((j * 7) % n_long) // (n_long - 1)
        out.append(entry(routing_header(hl, bool(j & 1), gid=base_gid + j, seed=j, silo=j % N_SILOS,
                                        ext="x%d" % j if j % 6 == 5 else None), bytes(range(j % 5)),
                         status=j % 2, host=(j + 1) % N_SILOS, act=j % N_ACT_KEYS, nk=j % 4))
    return out


def case_batches(cus: int, n: int = N_PIPE + 64) -> Case:
    smalls, longs = small_entries(), long_entries()
    _, _, stride, n_chunks = launch_shape(n, 8, cus)
    eidx, q0 = small_pattern(n, stride)
    k = 0
    for c in range(min(stride, n // 64)):
        for ln in spread_lanes(HELD_COUNTS[c % len(HELD_COUNTS)]):
            eidx[c * 64 + ln], q0[c * 64 + ln] = len(smalls) + k % len(longs), (k + k // len(longs)) % 4
            k += 1
    return Case("batches", smalls + longs, eidx, q0)


# d. the multi-chunk walk and the held list's overflow
WALK_WAVES = {5: (40, 40), 9: (64, 1), 13: (64, 64), 17: (20, 20)}   # wave -> long headers in its first and second chunk
WALK_OVERFLOWING = sorted(w for w, c in WALK_WAVES.items() if sum(c) > K_HELD_MAX)


def walk_n(cus: int) -> int:
    """2 * stride * 64 + 1 with stride = 8 * cus (three chunks for wave 0, the last one a single frame); on a device too
    small for that to reach the pipelined form, the smallest rounds * stride * 64 + 1 that does."""
    stride = 8 * cus
    rounds = max(2, -(-K_PIPE_MIN_FRAMES // (stride * 64)))
    return rounds * stride * 64 + 1


def case_walk(cus: int) -> Case:
    n = walk_n(cus)
    smalls = small_entries()
    longs = long_entries(19, 250, 1029, 5000) + long_entries(5, 1040, 4000, 5100) + [
        entry(routing_header(4300, True, gid=5200, seed=3), b"b", 0, host=3, act=2)]
    _, _, stride, _ = launch_shape(n, 8, cus)
    assert stride == 8 * cus
    eidx, q0 = small_pattern(n, stride)
    k = 0
    for w, counts in WALK_WAVES.items():
        for r, m in enumerate(counts):
            c = w + r * stride
            for ln in spread_lanes(m):
                eidx[c * 64 + ln], q0[c * 64 + ln] = len(smalls) + k % len(longs), (k + r + k // len(longs)) % 4
                k += 1
    return Case("walk", smalls + longs, eidx, q0)


# f. the buffer's end
def end_tail(mod: int) -> Tail:
    """Three valid frames whose bodies hold, in turn, a prefix whose body ends exactly at the buffer's end, a prefix
    whose body runs one byte past it, and eight zero bytes (hl = bl = 0 at nbytes - 8).  The offsets: the first
    frame, then 64 that all lie in the final 256 bytes or past them."""
    ha, hb, hc = (routing_header(MIN_LEN + k, bool(k), gid=6000 + k, seed=k) for k in range(3))
    la, lb, lc = 8 + len(ha) + 8, 8 + len(hb) + 8, 8 + len(hc) + 8
    total = la + lb + lc
    pa, pb = 8 + len(ha), la + 8 + len(hb)           # the two embedded prefixes
    fa = W.frame(ha, struct.pack("<ii", 0, total - pa - 8))
    fb = W.frame(hb, struct.pack("<ii", 0, total - pb - 8 + 1))
    fc = W.frame(hc, bytes(8))
    data = fa + fb + fc
    assert len(data) == total and total - pa <= 256
    offs = [("tail", 0), ("tail", la), ("tail", la + lb), ("tail", pa), ("tail", pb), ("end", -8), ("end", -7), ("end", 0),
            ("end", 1), ("abs", 2 ** 33)]
    k = 0
    while len(offs) < 65:   # arbitrary positions in the final 256 bytes: whatever the bytes there say
        offs.append(("end", -256 + 5 * k + 1))
        k += 1
    return Tail(data, offs, mod)


def case_end(cus: int, mod: int, n_body: int = N_PIPE - 1) -> Case:
    c = case_window(cus, n_body + 1)
    return Case("end%d" % mod, c.entries, c.eidx[:n_body], c.q0[:n_body], end_tail(mod))


# g. neighbour bytes: a header cut short whose body is the rest of it
CUT_LEN = 120
CUT_HELD_LEN, CUT_HELD_FROM = 400, 257      # cuts past byte 256: held rows
CUT_BIG_LEN, CUT_BIG_FROM = 1200, 1041      # cuts past byte 1,040: big[]


def cut_entries(L: int, first: int, grain_last: bool, gid: int) -> List[Entry]:
    h = routing_header(L, grain_last, gid=gid, seed=gid % 50)
    return [Entry(struct.pack("<ii", cut, L - cut) + h, route_word(cut % 2, cut % N_SILOS), cut % N_ACT_KEYS, cut % 4)
            for cut in range(first, L)]


def case_neighbour_short(n: int = N_PIPE) -> Case:
    """The 114 cuts of a 120-byte header (both variants), 128 bytes each, in four regions at the four alignments with
    no gap inside a region."""
    entries = cut_entries(CUT_LEN, 6, False, 7000) + cut_entries(CUT_LEN, 6, True, 7001)
    per = n // 4
    i = np.arange(n)
    region = np.minimum(i // per, 3)
    return Case("neighbour_short", entries, (i + region * 29) % len(entries), region)


def neighbour_long_specials() -> List[Tuple[Entry, int]]:
    held = cut_entries(CUT_HELD_LEN, CUT_HELD_FROM, True, 7100)
    big = cut_entries(CUT_BIG_LEN, CUT_BIG_FROM, True, 7200)
    return [(e, q) for q in range(4) for e in held + big]


def case_neighbour_long(cus: int, n: int = N_PIPE) -> Case:
    return _mixed("neighbour_long", n, cus, neighbour_long_specials(), per_chunk=40)


def specials_only(name: str, specials: List[Tuple[Entry, int]]) -> Case:
    """The specials alone, once each: a batch for the simple form."""
    return Case(name, [e for e, _ in specials], np.arange(len(specials)), [q for _, q in specials])


def all_cases(cus: int) -> List[Case]:
    return [case_window(cus), case_bounds(cus), case_batches(cus), case_walk(cus)] + [case_end(cus, m) for m in range(4)] + [
        case_neighbour_short(), case_neighbour_long(cus)]
