"""The directory partition's probe chains on small, crowded tables: the key families of tests/dir_layout.py against the
library's own slot function, and the host mirror alone (device = -1) against the oracle's unordered_map partition at
2, 8, 64 and 4096 slots.  The GPU scenarios over the same families are in test_gpu_dir_edges.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dir_layout as D
from oracle import cpu_ref
from orleans_amd import _lib as L
from orleans_amd import workloads as W
from orleans_amd.engine import GrainDirectoryEngine, OrleansRouteError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SILOS = 8

HOST_PROGRAM = r"""
#include <cstdio>
#include "orl_internal.h"
int main() {
    const unsigned long long masks[5] = {1, 7, 63, 4095, (1ull << 20) - 1};
    unsigned long long x = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 400; ++i) {
        unsigned long long k[3];
        for (auto& v : k) { x = x * 6364136223846793005ull + 1442695040888963407ull; v = x ^ (x >> 29); }
        if (i % 3 == 0) k[1] = 0;                      // long keys, as the families use
        if (i % 6 == 0) k[2] &= 0xFFFFFFFFull;
        const uint32_t h = orl::jenkins3(k[0], k[1], k[2]);
        std::printf("%llu %llu %llu %u %u", k[0], k[1], k[2], h, orl::fmix32(h));
        for (auto m : masks) std::printf(" %llu", (unsigned long long)orl::dir_slot(h, m));
        std::printf("\n");
    }
}
"""


def test_numpy_slot_function_equals_the_header(tmp_path):
    """jenkins3, fmix32 and dir_slot of orl_internal.h, compiled for the host, against their numpy restatements
    (workloads.jenkins3_np, dir_layout.fmix32_np / dir_slot_np) for 400 keys and masks 1, 7, 63, 4095 and 2^20 - 1: if the
    slot function ever changes, the families stop being adversarial and this test says so."""
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("no hipcc")
    src, exe = tmp_path / "slots.cpp", tmp_path / "slots"
    src.write_text(HOST_PROGRAM)
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I",
                        os.path.join(ROOT, "orleans_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rows = np.array([[int(v) for v in line.split()] for line in out.stdout.splitlines()], dtype=np.uint64)
    assert rows.shape == (400, 10)
    h = W.jenkins3_np(rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy())
    np.testing.assert_array_equal(h, rows[:, 3].astype(np.uint32))
    np.testing.assert_array_equal(D.fmix32_np(h), rows[:, 4].astype(np.uint32))
    for j, slots in enumerate((2, 8, 64, 4096, 1 << 20)):
        np.testing.assert_array_equal(D.dir_slot_np(h, slots), rows[:, 5 + j].astype(np.int64))
        assert len(np.unique(rows[:, 5 + j])) > 1


@pytest.fixture(scope="module")
def cluster():
    return W.default_cluster(N_SILOS)


@pytest.mark.parametrize("slots", D.SIZES)
def test_family_conditions(cluster, slots):
    """Every family at every size: exactly slots / 2 distinct keys that keep the 8-B probe form, start slots as named,
    ghosts and aliases disjoint from the keys, and for tail(w) m > w keys, so at least m - w entries wrap."""
    tcd = W.grain_tcd(cluster)
    names = D.family_names(slots)
    assert "random" in names and f"one_slot({slots - 1})" in names and "line_edge(32)" in names
    assert ("tail(4)" in names) == (slots >= 64) and ("tail(1)" in names) == (slots >= 8)
    for name in names:
        f = D.family(name, slots, tcd)
        f.check()
        if f.wrap_window:
            assert f.min_wrapped() == len(f.keys) - f.wrap_window or slots == 2
    ck = D.control_keys(tcd, 16)
    assert ck["n1"].min() > D.SCAN_LONG


def test_keyext_family_conditions(cluster):
    tcd = W.grain_tcd(cluster, L.CAT_KEYEXT_GRAIN)
    for name in D.keyext_family_names():
        reg, ghosts, start = D.keyext_family(name, tcd)
        assert len(set(reg)) == len(reg) and not set(reg) & set(ghosts) and len(ghosts) >= 4
        assert len(start) == len(reg)


def _oracle(cluster):
    o = cpu_ref.Oracle(N_SILOS, seed=0)
    for s in range(N_SILOS):
        o.add_server(s, int(cluster.hashes[s]))
    return o


def _check_lookup(eng, o, keys):
    """lookup_host of every key against the oracle: a message from silo 0 hits exactly the registered keys (every silo is
    local and functional here), with the same activation handle and host silo."""
    a, s = eng.lookup_host(keys)
    r, act = o.route(D.messages(keys, 1))
    hit = ((r >> 16) & 0xFF) == L.ST_HIT
    np.testing.assert_array_equal(a != L.NO_ACT, hit)
    np.testing.assert_array_equal(a[hit], act[hit])
    np.testing.assert_array_equal(s[hit], ((r >> 8) & 0xFF).astype(np.uint8)[hit])
    assert (s[~hit] == 0xFF).all()
    assert eng.directory_count() == o.size()


@pytest.mark.parametrize("slots", D.SIZES)
def test_host_mirror_crowded_vs_oracle(cluster, slots):
    """The host mirror alone (orl_api.cpp dir_find and its insert / remove), every family: registered to exactly half
    load, one key more refused with E_CAPACITY and nothing changed, every other key unregistered (tombstones inside the
    chains), everything looked up, the mirror compacted, the removed keys re-registered with new handles — statuses,
    winners, removed flags, lookups and the count equal to the oracle's after every step.  Whether a registration is
    refused is the documented rule (count + tombstones + 1) * 2 > slots, evaluated here from the counts at each step."""
    tcd = W.grain_tcd(cluster)
    for name in D.family_names(slots):
        f = D.family(name, slots, tcd)
        f.check()
        m = len(f.keys)
        everything = np.concatenate([f.keys, f.ghosts, f.aliases])
        eng = GrainDirectoryEngine(n_act=1 << 20, dir_capacity=slots // 2, max_batch=1024, device=-1)
        W.setup_engine(eng, cluster)
        o = _oracle(cluster)
        count = tombs = 0

        def refused(count, tombs):
            return (count + tombs + 1) * 2 > slots

        acts = np.arange(m, dtype=np.uint32) + 100
        silos = (np.arange(m) % N_SILOS).astype(np.uint8)
        assert not refused(m - 1, 0)
        st, wa, ws = eng.register_single_activation(f.keys, acts, silos)
        st_o, wa_o, ws_o = o.register(f.keys, acts, silos)
        np.testing.assert_array_equal(st, st_o)
        np.testing.assert_array_equal(wa, wa_o)
        np.testing.assert_array_equal(ws, ws_o)
        assert (st == L.INS_INSERTED).all()
        count = m
        assert eng.directory_count() * 2 == slots
        _check_lookup(eng, o, everything)
        # one key more: refused, nothing changes; a registered key again is EXISTING whatever the load
        assert refused(count, tombs)
        with pytest.raises(OrleansRouteError) as e:
            eng.register_single_activation(f.ghosts[:1], np.array([7], np.uint32), np.zeros(1, np.uint8))
        assert e.value.code == L.E_CAPACITY, (name, e.value)
        _check_lookup(eng, o, everything)
        st, wa, _ = eng.register_single_activation(f.keys[-1:], np.array([9], np.uint32), np.zeros(1, np.uint8))
        st_o, wa_o, _ = o.register(f.keys[-1:], np.array([9], np.uint32), np.zeros(1, np.uint8))
        assert (st[0], wa[0]) == (st_o[0], wa_o[0]) == (L.INS_EXISTING, acts[-1])
        # every other key out (also a ghost and an alias: not there)
        gone = np.concatenate([f.keys[::2], f.ghosts[:1], f.aliases[:1]])
        rm = eng.unregister(gone)
        np.testing.assert_array_equal(rm, o.unregister(gone))
        n_gone = int(rm.sum())
        assert n_gone == len(f.keys[::2])
        count, tombs = count - n_gone, tombs + n_gone
        _check_lookup(eng, o, everything)
        # the removed keys again, new handles: the rule decides whether the mirror takes them before a compaction
        back = f.keys[::2]
        acts2 = np.arange(len(back), dtype=np.uint32) + 5000
        silos2 = ((np.arange(len(back)) + 3) % N_SILOS).astype(np.uint8)
        if refused(count, tombs):
            with pytest.raises(OrleansRouteError) as e:
                eng.register_single_activation(back, acts2, silos2)
            assert e.value.code == L.E_CAPACITY, (name, e.value)
            _check_lookup(eng, o, everything)
            eng.compact_directory()
            tombs = 0
            _check_lookup(eng, o, everything)
        assert not refused(count + len(back) - 1, tombs)
        st, wa, ws = eng.register_single_activation(back, acts2, silos2)
        st_o, wa_o, ws_o = o.register(back, acts2, silos2)
        np.testing.assert_array_equal(st, st_o)
        np.testing.assert_array_equal(wa, wa_o)
        np.testing.assert_array_equal(ws, ws_o)
        assert (st == L.INS_INSERTED).all()
        count += len(back)
        assert count * 2 == slots and eng.directory_count() == count
        _check_lookup(eng, o, everything)
        eng.compact_directory()
        _check_lookup(eng, o, everything)
        eng.close()
