"""The scan-shaped device code keeps its shared helpers in one place, and the case lists of the GPU tests
reach the chunked regime of the one-workgroup tile scan for the constants that header holds.  The host side is cut into
units by subsystem behind one private context header.  Text files only: no GPU."""
import os
import re

import admission_ref as A
import collector_ref as R
import completion_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orleans_amd", "csrc")
HEADER = "tile_scan_dev.h"

SHARED = ("block_exclusive", "tile_scan_body", "bucket_of", "bucket_keys", "load_bytes", "store_bytes", "load_words",
          "load_order", "stream_words", "stream_bytes", "BlockCounts")


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC))}


def _definitions(name, text):
    """Definitions of a function (a return type, the name, a parameter list, a body) or of a struct."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    fn = re.findall(r"^[ \t]*(?:[\w:<>*&,]+[ \t]+)+[*&]?%s\s*\([^;{}]*\)\s*(?:const\s*)?\{" % name, text, flags=re.M)
    return len(fn) + len(re.findall(r"\bstruct\s+%s\s*\{" % name, text))


def test_shared_scan_helpers_are_defined_once_in_the_header():
    src = _sources()
    for name in SHARED:
        where = [f for f, text in src.items() if _definitions(name, text)]
        assert where == [HEADER] and _definitions(name, src[HEADER]) == 1, (name, where)
    # no file fell back to a block scan of its own under DESIGN §19's acceptance rule
    assert not [f for f, text in src.items() if _definitions("block_scan_256", text)]


def test_the_regex_sees_a_definition():
    text = "template <class T>\n__device__ __forceinline__ T* f(T v, int (&a)[8]) {\n}\nstruct G {\n};\nint h(int);\n x = f(1, a);"
    assert (_definitions("f", text), _definitions("G", text), _definitions("h", text)) == (1, 1, 0)


def test_the_host_side_does_not_include_the_device_header():
    src = _sources()
    users = {f for f, text in src.items() if re.search(r'#include\s+"%s"' % re.escape(HEADER), text)}
    assert users == {"admit.hip", "waitq.hip", "collect.hip", "cache_evict.hip", "cache_adaptive.hip"}, users
    host = [f for f in src if f.endswith(".cpp")]
    assert "orl_node.cpp" in host and len(host) >= 6, host
    for f in host:  # nor through a header of theirs, to any depth
        seen, todo = set(), [f]
        while todo:
            for inc in re.findall(r'#include\s+"([^"]+)"', src[todo.pop()]):
                assert os.path.basename(inc) not in users and inc != HEADER, (f, inc)
                if inc in src and inc not in seen:
                    seen.add(inc)
                    todo.append(inc)


# ---- the host side's layout ------------------------------------------------------------------------------
CTX_HEADER = "orl_ctx.h"


def test_the_context_struct_is_defined_once_in_its_header():
    src = _sources()
    where = {f: len(re.findall(r"\bstruct\s+orl_ctx\s*\{", text)) for f, text in src.items()}
    assert {f: n for f, n in where.items() if n} == {CTX_HEADER: 1}, where


def test_no_device_unit_includes_the_context_header():
    src = _sources()
    users = {f for f, text in src.items() if re.search(r'#include\s+"%s"' % re.escape(CTX_HEADER), text)}
    assert users and all(f.endswith(".cpp") for f in users), users  # no .hip file, and no header a .hip file may include
    assert "orl_node.cpp" not in users  # it keeps to the orl::ctx_* accessors


def test_every_declared_entry_point_is_defined_in_exactly_one_unit():
    header = open(os.path.join(ROOT, "include", "orleans_route.h")).read()
    header = re.sub(r"/\*.*?\*/|//[^\n]*", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(orl_\w+)\s*\([^;{}]*\)\s*;", header)))
    assert len(declared) > 100 and "orl_ctx_create" in declared and "orl_collect_scan_all_device" in declared, len(declared)
    units = {f: text for f, text in _sources().items() if f.endswith((".cpp", ".hip"))}
    for name in declared:
        where = {f: _definitions(name, text) for f, text in units.items() if _definitions(name, text)}
        assert len(where) == 1 and list(where.values()) == [1], (name, where)


def test_no_file_closes_and_reopens_extern_c():
    for f, text in _sources().items():
        assert len(re.findall(r'extern\s+"C"\s*\{', text)) <= 1, f
        if f.startswith("api_"):  # and a unit cut out of orl_api.cpp keeps its private helpers in one anonymous namespace
            assert len(re.findall(r"^namespace\s*\{", text, flags=re.M)) <= 1, f


def _constant(name):
    m = re.search(r"constexpr uint32_t %s = (\d+);" % name, open(os.path.join(CSRC, HEADER)).read())
    assert m, name
    return int(m.group(1))


def test_gpu_case_lists_reach_the_chunked_tile_scan():
    """The shapes of the three test_chunked_tile_scan tests: as many tiles as the scan workgroup has threads (chunk 1,
    every thread busy), one tile more (chunk 2, the last working thread owns one aggregate) and chunk 3."""
    tile, threads = _constant("kTileThreads") * _constant("kTileItems"), _constant("kScanThreads")
    assert A.CHUNK_STRIDE % tile != 0 and A.CHUNK_STRIDE > tile  # every bucket crosses a tile edge; heads lie off them
    for shapes in (A.CHUNK_N, Q.CHUNK_N, R.CHUNK_N_ACT):
        ntiles = [(n + tile - 1) // tile for n in shapes]
        chunk = [(t + threads - 1) // threads for t in ntiles]
        assert chunk == [1, 2, 3], (shapes, chunk)
        assert ntiles[0] == threads and ntiles[1] == threads + 1 and ntiles[1] % 2 == 1 and ntiles[2] > 2 * threads
        assert all(n % tile == 1 for n in shapes[1:])  # and the last tile holds one item
    assert set(R.CHUNK_DENSITIES) == {"one-per-tile", "all"}


def test_chunk_builders_agree_with_the_loops_at_a_small_size():
    """The builders of those tests at n = 3 buckets and one position, where the sequential models are quick: the numpy
    forms the GPU tests compare against give what the loops give."""
    import numpy as np
    n = 3 * A.CHUNK_STRIDE + 1
    for sc in A.chunk_scenarios(n):
        d1, s1, c1 = sc.expect()
        d2, s2, c2 = A.admit_closed_form(sc.act, sc.mflags, sc.state, sc.n_act, sc.hard, sc.hard_stateless)
        assert np.array_equal(d1, d2) and np.array_equal(s1, s2) and list(c1) == list(c2), sc.name
        assert len(set(d1.tolist()) & {0, 1, 2}) >= 2, sc.name
    for name, w, act, tok, fl, disp in Q.chunk_appends(n):
        assert Q.append_ref(w, act, tok, fl, disp).same(Q.append(w, act, tok, fl, disp)), name
    for name, w, cact, ctok in Q.chunk_completes(n):
        w.check_invariants()
        l_w, l_out, l_counts = Q.complete(w, cact, ctok)
        c_w, c_out, c_counts = Q.complete_closed_form(w, cact, ctok)
        assert c_w.same(l_w) and sorted(c_out) == sorted(l_out) and list(c_counts) == list(l_counts), name
        a_out = Q.complete_closed_form(w, cact, ctok, as_arrays=True)[1]
        assert [tuple(int(x) for x in o) for o in zip(*a_out)] == c_out and len(c_out) > 0, name
