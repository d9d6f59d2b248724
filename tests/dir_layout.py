"""Key sets with a chosen start slot in the directory's open-addressed tables.  TEST INFRASTRUCTURE ONLY.

Every routed message ends in a linear-probe walk that starts at ``dir_slot(jenkins3(key), mask)`` (orl_internal.h):
``slot = (fmix32(jenkins3(tcd, n0, n1)) * slots) >> 32``.  This module restates that in numpy (test_dir_layout.py checks
the restatement against the header itself) and scans long keys N1 = 1, 2, ... of one type code for families whose start
slots are where the walks are most likely to be wrong:

    tail(w)        every key starts in the last w slots (w = 1, 4): with m > w keys at least m - w entries wrap
    one_slot(s)    every key starts at slot s (0, slots / 2, slots - 1): one chain of slots / 2 entries
    line_edge(b)   every start slot is the last slot of a 64-B line of b-byte slots (index = 1 mod 2 for the 32-B table,
                   3 mod 4 for the 16-B probe table, 7 mod 8 for the 8-B one): the first step crosses a line
    random         the control: the first keys of the scan, whatever their slot

Every family holds exactly slots / 2 keys (the partition's full load), `ghosts` (keys of the same start slots that are
never registered) and `aliases` (N1 + 2^32 of registered keys: the same low 32 bits, so the 8-B probe form must miss
them).  N1 stays below 2^32 - 2 and handles below 2^24, so a table of these keys keeps the 8-B probe form.

The KeyExt families do the same over the KeyExt table's hash, scanning the extensions "k0", "k1", ...
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import List, Tuple

import numpy as np

from orleans_amd import _lib as L
from orleans_amd.workloads import jenkins3_np

SIZES = (2, 8, 64, 4096)          # slots; dir_capacity = slots / 2
SCAN = 1 << 20                    # candidates N1 = 1 .. SCAN (a single start slot of 4096 needs the long scan)
SCAN_LONG = 1 << 24
CONTROL_BASE = 1 << 26            # N1 of the control keys a scenario adds to a family (disjoint from every scan)
ALIAS = np.uint64(1 << 32)
MAX_GHOSTS = 64


def fmix32_np(h: np.ndarray) -> np.ndarray:
    """murmur3's finalizer (orl_internal.h fmix32) over a uint32 array."""
    h = np.asarray(h, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def dir_slot_np(h: np.ndarray, slots: int) -> np.ndarray:
    """orl_internal.h dir_slot for a table of `slots` slots (mask = slots - 1): the high bits of fmix32(h)."""
    return ((fmix32_np(h).astype(np.uint64) * np.uint64(slots)) >> np.uint64(32)).astype(np.int64)


def start_slots(keys: np.ndarray, slots: int) -> np.ndarray:
    """Start slot of every key (KEY_DTYPE) in a partition of `slots` slots."""
    return dir_slot_np(jenkins3_np(keys["tcd"], keys["n0"], keys["n1"]), slots)


@lru_cache(maxsize=None)
def _scan_hashes(tcd: int, n: int, base: int = 0) -> np.ndarray:
    """jenkins3 of the long keys N1 = base + 1 .. base + n of type `tcd` (index i holds N1 = base + i + 1)."""
    n1 = np.arange(base + 1, base + n + 1, dtype=np.uint64)
    return jenkins3_np(np.full(n, tcd, np.uint64), np.zeros(n, np.uint64), n1)


@dataclass
class Family:
    name: str
    slots: int
    keys: np.ndarray      # KEY_DTYPE, exactly slots / 2: the registered keys
    ghosts: np.ndarray    # KEY_DTYPE: same start slots, never registered
    aliases: np.ndarray   # KEY_DTYPE: N1 + 2^32 of registered keys, never registered
    start: np.ndarray     # start slot of every key of `keys`
    wrap_window: int      # w for tail(w) and one_slot(slots - 1) (1), else 0

    def check(self) -> None:
        """The conditions a scenario relies on, asserted rather than assumed."""
        s, m = self.slots, len(self.keys)
        assert m * 2 == s, (self.name, s, m)
        assert len(np.unique(self.keys["n1"])) == m and (self.keys["n0"] == 0).all()
        assert (self.keys["n1"] < np.uint64((1 << 32) - 2)).all() and (self.keys["n1"] > 0).all()
        np.testing.assert_array_equal(self.start, start_slots(self.keys, s))
        if len(self.ghosts):
            assert not np.isin(self.ghosts["n1"], self.keys["n1"]).any()
        assert len(self.ghosts) + len(self.aliases) > 0
        np.testing.assert_array_equal(self.aliases["n1"] & np.uint64(0xFFFFFFFF), self.keys["n1"][: len(self.aliases)])
        assert (self.aliases["n1"] >> np.uint64(32) == 1).all()
        kind = self.name.split("(")[0]
        if kind == "tail":
            w = self.wrap_window
            assert m > w, "pigeonhole: m keys in the last w slots wrap at least m - w entries"
            assert (self.start >= s - w).all()
            assert self.min_wrapped() >= m - w > 0
        elif kind == "one_slot":
            assert len(np.unique(self.start)) == 1
        elif kind == "line_edge":
            per_line = 64 // int(self.name[10:-1])
            assert (self.start % per_line == per_line - 1).all()

    def min_wrapped(self) -> int:
        """Entries of the fully registered family that lie past the table's last slot (in slots 0, 1, ...), whatever the
        insertion order: the slots from the lowest start slot to the end hold at most one entry each."""
        return max(0, len(self.keys) - (self.slots - int(self.start.min())))


def family_names(slots: int) -> List[str]:
    """The families that exist at this table size.  A table holds slots / 2 keys, so tail(w) (m > w keys) needs
    slots / 2 > w, and line_edge(b) needs a whole 64-B line (64 / b slots); families that would repeat another one at
    this size (one_slot(slots / 2) = one_slot(slots - 1) at 2 slots) are listed once."""
    names = ["random"]
    for w in (1, 4):
        if slots // 2 > w:
            names.append(f"tail({w})")
    for s in dict.fromkeys((0, slots // 2, slots - 1)):
        names.append(f"one_slot({s})")
    for b in (32, 16, 8):
        if slots >= 64 // b:
            names.append(f"line_edge({b})")
    return names


def _keys(tcd: int, n1: np.ndarray) -> np.ndarray:
    out = np.zeros(len(n1), L.KEY_DTYPE)
    out["tcd"] = np.uint64(tcd)
    out["n1"] = np.asarray(n1, np.uint64)
    return out


@lru_cache(maxsize=None)
def family(name: str, slots: int, tcd: int) -> Family:
    """The family `name` (see family_names) for a partition of `slots` slots and long keys of TypeCodeData `tcd`."""
    m = slots // 2
    kind = name.split("(")[0]
    arg = int(name[len(kind) + 1:-1]) if "(" in name else 0
    for scan in (SCAN, SCAN_LONG):
        slot = dir_slot_np(_scan_hashes(tcd, scan), slots)
        if kind == "random":
            sel = np.ones(scan, bool)
        elif kind == "tail":
            sel = slot >= slots - arg
        elif kind == "one_slot":
            sel = slot == arg
        elif kind == "line_edge":
            per_line = 64 // arg
            sel = slot % per_line == per_line - 1
        else:
            raise ValueError(name)
        idx = np.nonzero(sel)[0]
        if len(idx) >= m + min(MAX_GHOSTS, max(4, m)):
            break
    assert len(idx) > m, (name, slots, len(idx))
    n1 = (idx + 1).astype(np.uint64)
    keys = _keys(tcd, n1[:m])
    ghosts = _keys(tcd, n1[m: m + MAX_GHOSTS])
    aliases = _keys(tcd, keys["n1"][:MAX_GHOSTS] + ALIAS)
    wrap = arg if kind == "tail" else 1 if name == f"one_slot({slots - 1})" else 0
    f = Family(name, slots, keys, ghosts, aliases, slot[idx[:m]], wrap)
    assert (start_slots(ghosts, slots) == slot[idx[m: m + len(ghosts)]]).all()
    return f


def control_keys(tcd: int, n: int) -> np.ndarray:
    """n long keys of the same type that no family and no ghost list holds (N1 above every scan), random start slots."""
    return _keys(tcd, np.arange(CONTROL_BASE + 1, CONTROL_BASE + n + 1, dtype=np.uint64))


def messages(keys: np.ndarray, n_silos: int, seed: int = 0) -> np.ndarray:
    """One Application message per key, sending silos cycling from `seed`."""
    msgs = np.zeros(len(keys), L.MSG_DTYPE)
    msgs["tcd"], msgs["n0"], msgs["n1"] = keys["tcd"], keys["n0"], keys["n1"]
    msgs["sending_silo"] = ((np.arange(len(keys)) + seed) % n_silos).astype(np.uint8)
    msgs["category"] = 2
    return msgs


# ---- KeyExt table -----------------------------------------------------------------------------------------------------
# The context's KeyExt table is never smaller than 1024 slots (orl_api.cpp ext_rebuild starts at 1024 and doubles), so the
# KeyExt families are built for that size rather than for 64 slots; they hold fewer than 512 keys, which keeps the table
# at its initial size through every step (host inserts rebuild at (entries + tombstones + 1) * 2 > slots).
KEYEXT_SLOTS = 1024
KEYEXT_SCAN = 1 << 16


@lru_cache(maxsize=None)
def _keyext_scan(tcd: int, n1: int) -> np.ndarray:
    """KeyExt uniform hash of (tcd, 0, n1, "k%d") for d in [0, KEYEXT_SCAN), by the oracle's pyref.uniform_hash."""
    from oracle import pyref as P
    return np.array([P.uniform_hash(P.Key(tcd, 0, n1, "k%d" % d)) for d in range(KEYEXT_SCAN)], np.uint32)


def keyext_family_names() -> List[str]:
    s = KEYEXT_SLOTS
    return ["random", "tail(1)", "tail(4)", "one_slot(0)", f"one_slot({s // 2})", f"one_slot({s - 1})"]


def keyext_family(name: str, tcd: int, n1: int = 7) -> Tuple[List[str], List[str], np.ndarray]:
    """(registered extensions, ghost extensions, start slots of the registered ones) of the KeyExt family `name` over
    grains (tcd, 0, n1, "k%d").  tail(w) holds more than w keys; a one_slot family holds every candidate of its slot
    but the ghosts (about 64 candidates per slot in the scan)."""
    slots = KEYEXT_SLOTS
    slot = dir_slot_np(_keyext_scan(tcd, n1), slots)
    kind = name.split("(")[0]
    arg = int(name[len(kind) + 1:-1]) if "(" in name else 0
    if kind == "random":
        idx = np.arange(200)
    elif kind == "tail":
        idx = np.nonzero(slot >= slots - arg)[0]
    else:
        idx = np.nonzero(slot == arg)[0]
    n_ghost = max(4, len(idx) // 4)
    reg, ghost = idx[:-n_ghost], idx[-n_ghost:]
    assert len(reg) > 8 and len(reg) < slots // 2, (name, len(idx))
    if kind == "tail":
        assert len(reg) > arg and (slot[reg] >= slots - arg).all()
    if kind == "one_slot":
        assert (slot[reg] == arg).all() and (slot[ghost] == arg).all()
    return ["k%d" % d for d in reg], ["k%d" % d for d in ghost], slot[reg]
