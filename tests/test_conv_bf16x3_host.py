"""The host-side decisions of the bf16x3 conv family (csrc/conv1d_bf16x3.hip), pinned shape by shape: tests/golden/conv_bf16x3_host.json holds what
a library answered (tools/gen_golden_conv_host.py: split counts and workspace sizes at 256 CUs, partial-sum rows, plane rows, packed-weight sizes, and
the status and message of calls the argument checks reject); the current library must give every entry again, exactly.

Host code only, by construction: the queries launch nothing, and every recorded call of a launching entry point is one that was refused — a
refusal here is asserted before the answer is compared, so a call that WOULD launch fails the test on its status.  Runs on the simulator build
and, without a GPU, on the gfx950 library (as tests/test_abi.py does)."""
import ctypes
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_table = None


def _golden():
    global _table
    if _table is None:
        with open(os.path.join(HERE, "golden", "conv_bf16x3_host.json")) as f:
            _table = json.load(f)
    return _table


def _gfx950_lib():
    from test_abi import _ensure_built
    return _ensure_built().load()


@pytest.fixture(params=("sim", "gfx950"))
def lib(request):
    return request.getfixturevalue("emu").lib if request.param == "sim" else _gfx950_lib()


def test_table_covers_the_issue_s_cases():
    t = _golden()
    assert t["cus"] == 256 and t["splits"] == [-1, 0, 2, 3, 16, 64, 65]
    shapes = [s for s, _ in t["split"]]
    assert {s[0] for s in shapes} >= {0, 1, 2}
    assert {s[3] for s in shapes} >= {1, 2, 64, 65, 128, 129} and {s[4] for s in shapes} >= {1, 127, 128, 129, 260}
    assert {s[5] for s in shapes} >= set(range(1, 10)) and {s[6] for s in shapes} >= {1, 2, 3, 4, 8, 16, 64, 128}
    assert {s[7] for s in shapes} >= {1, 3, 9, 12} and {s[1] for s in shapes} >= {1, 2}
    for flagship in ([0, 1, 1024, 2048, 1024, 16, 8, 1, 4], [0, 1, 2048, 128, 1024, 3, 1, 1, 1], [2, 1, 2048, 64, 1024, 7, 1, 1, 3]):
        assert flagship in shapes
    assert {r[0] for r in t["refusals"]} == {"sat_conv1d_bf16x3", "sat_conv1d_bf16x3_emit", "sat_conv1d_bf16x3_ws", "sat_conv1d_bf16x3_planesq",
                                             "sat_conv1d_bf16x3_planesq_ws", "sat_residual_unit_fwd", "sat_convtr1d_bf16x3", "sat_convtr1d_bf16x3_ws"}
    assert all(r[4] != 0 for r in t["refusals"])


def test_split_counts_and_workspaces(lib):
    t = _golden()
    bad = []
    for shape, row in t["split"]:
        for want, (n, ws) in zip(t["splits"], row):
            need = ctypes.c_longlong(-7)
            got = [lib.sat_conv_bf16x3_split(*shape, want, t["cus"], ctypes.byref(need)), need.value]
            if got != [n, ws]:
                bad.append((shape, want, got, [n, ws]))
    assert not bad, bad[:10]


@pytest.mark.parametrize("key,fn", [("conv_rows", "sat_conv1d_bf16x3_partial_rows"), ("convtr_rows", "sat_convtr1d_bf16x3_partial_rows"),
                                    ("plane_rows", "sat_conv1d_k7_plane_rows"), ("pack_size", "sat_pack_weights_bf16x3_size"),
                                    ("pack_k7q_size", "sat_pack_weights_k7q_size")])
def test_queries(lib, key, fn):
    rows = _golden()[key]
    assert len(rows) > 100
    bad = [(r, got) for r in rows for got in [getattr(lib, fn)(*r[:-1])] if got != r[-1]]
    assert not bad, bad[:10]


def test_refusals(lib):
    """status and message (after the entry point's name) of every rejected call; the message names the library's own entry point"""
    tools = os.path.join(os.path.dirname(HERE), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    from gen_golden_conv_host import call_refusal
    bad = []
    for name, nptr, ints, tail, status, text in _golden()["refusals"]:
        got = call_refusal(lib, name, nptr, ints, tail)
        if got != (status, text):
            bad.append((name, ints, tail, got, (status, text)))
    assert not bad, bad[:10]
