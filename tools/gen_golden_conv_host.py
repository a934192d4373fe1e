#!/usr/bin/env python
"""The host-side answers of the bf16x3 conv family (csrc/conv1d_bf16x3.hip), shape by shape -> tests/golden/conv_bf16x3_host.json, which
tests/test_conv_bf16x3_host.py replays against the current library and compares entry for entry.  Run it on a library built from the commit
whose answers are to be pinned (the parent of a change to that host code):

    python tools/gen_golden_conv_host.py --lib path/to/libsat_amd.so      (or a simulator build, libsat_emu.so: the host code is the same)

Every call is host code only:
  split            sat_conv_bf16x3_split(kind 0 | 1 | 2, ..., split, cus = 256, &ws_floats) for split in SPLITS -> [count, ws_floats]
  conv_rows        sat_conv1d_bf16x3_partial_rows(B, Tout, K, stride)
  convtr_rows      sat_convtr1d_bf16x3_partial_rows(B, Tout, stride, pad)
  plane_rows       sat_conv1d_k7_plane_rows(Tin, Tout, pad)
  pack_size        sat_pack_weights_bf16x3_size(D0, D1, K, stride, mode)
  pack_k7q_size    sat_pack_weights_k7q_size(D0, D1, K, mode)
  refusals         the launching entry points with NULL for every pointer and arguments that are rejected before anything is launched:
                   [name, [the integer arguments, in order], status, sat_last_error() after the entry point's name].  A non-zero status is
                   asserted before an entry is recorded.  No argument set that could reach a launch belongs here: with NULL planes a legal
                   plane-fed shape is left out as well.
Shapes: the conv launches of the flagship generator step (tests/test_conv_split.py::test_rule_on_the_flagship_step) and small edge cases —
Cout 1, 2, 64, 65, 128, 129; Tout 1, 127, 128, 129, 260; K 1 .. 9; strides 1, 2, 3, 4, 8, 16, 64, 128; dilations 1, 3, 9, 12; B 1 and 2."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from stable_audio_tools_amd import _lib       # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "conv_bf16x3_host.json")
CUS = 256
SPLITS = (-1, 0, 2, 3, 16, 64, 65)
COUTS = (1, 2, 64, 65, 128, 129)
TOUTS = (1, 127, 128, 129, 260)
KS = tuple(range(1, 10))
STRIDES = (1, 2, 3, 4, 8, 16, 64, 128)
DILS = (1, 3, 9, 12)
BS = (1, 2)


def flagship_shapes():
    """(kind, B, Cin, Cout, Tout, K, stride, dil, pad): batch 1, 2097152 samples, channels 128 x (1, 2, 4, 8, 16), strides (2, 4, 4, 8, 8)"""
    out = [(0, 1, 1024, 2048, 1024, 16, 8, 1, 4), (0, 1, 2048, 128, 1024, 3, 1, 1, 1), (2, 1, 2048, 64, 1024, 7, 1, 1, 3),
           (1, 1, 2048, 1024, 8192, 16, 8, 1, 4), (0, 1, 128, 2048, 1024, 3, 1, 1, 1), (2, 1, 64, 2048, 1024, 7, 1, 1, 3),
           (0, 1, 2048, 128, 1024, 7, 1, 1, 3)]
    for cin, cout, s, tout in ((128, 128, 2, 1048576), (128, 256, 4, 262144), (256, 512, 4, 65536), (512, 1024, 8, 8192)):
        out.append((0, 1, cin, cout, tout, 2 * s, s, 1, (s + 1) // 2))
        out.append((1, 1, cout, cin, tout * s, 2 * s, s, 1, (s + 1) // 2))
    for c, t in ((128, 2097152), (128, 1048576), (256, 262144), (512, 65536), (1024, 8192)):
        out.append((0, 1, c, c, t, 1, 1, 1, 0))
        out += [(2, 1, c, c, t, 7, 1, d, 3 * d) for d in (1, 3, 9)]
    return out


def edge_shapes():
    out = []
    for b in BS:
        for cout in COUTS:
            for tout in TOUTS:
                out.append((0, b, 256, cout, tout, 3, 1, 1, 1))            # plan (8, 2)
                out.append((0, b, 512, cout, tout, 1, 1, 1, 0))            # plan (4, 4)
                out.append((0, b, 64, cout, tout, 16, 8, 1, 4))            # strided
                out.append((1, b, 512, cout, tout, 4, 2, 1, 1))            # transposed
                out.append((2, b, 256, cout, tout, 7, 1, 1, 3))            # planes
    for k in KS:
        for dil in DILS:
            out.append((0, 2, 256, 64, 260, k, 1, dil, (k - 1) * dil // 2))
            out.append((2, 2, 256, 64, 260, k, 1, dil, min((k - 1) * dil // 2, 40)))
    for s in STRIDES:
        for dil in (1, 3):
            out.append((0, 1, 64, 128, 129, 2 * s, s, dil, (s + 1) // 2))
        out.append((0, 1, 64, 128, 129, 7, s, 1, 3))
        out.append((1, 2, 512, 65, 260, 2 * s, s, 1, (s + 1) // 2))
        out.append((1, 2, 512, 65, 260, 2 * s + 1, s, 1, 0))
        out.append((2, 1, 512, 64, 129, 7, s, 1, 3))
    out += [(0, 0, 64, 64, 128, 3, 1, 1, 1), (0, 1, 0, 64, 128, 3, 1, 1, 1), (0, 1, 64, 0, 128, 3, 1, 1, 1), (0, 1, 64, 64, 0, 3, 1, 1, 1),
            (1, 1, 64, 64, 128, 4, 2, 1, -1), (2, 1, 256, 64, 128, 7, 1, 1, 33), (2, 1, 256, 64, 128, 7, 1, 1, -1), (2, 1, 256, 64, 128, 7, 1, 0, 3),
            (3, 1, 128, 128, 128, 7, 1, 1, 3), (-1, 1, 128, 128, 128, 7, 1, 1, 3), (0, 1, 4096, 64, 128, 3, 1, 1, 1)]
    return out


def refusal_calls(lib):
    """(name, number of leading pointers, ints, trailing arguments after the ints) — trailing None = a NULL pointer.  Every set is rejected by the
    argument checks, or by the split decision, which both come before a launch."""
    rows7 = lib.sat_conv1d_k7_plane_rows(260, 260, 3)
    conv_bad = [(0, 8, 8, 64, 64, 3, 1, 1, 1, 0), (1, 0, 8, 64, 64, 3, 1, 1, 1, 0), (1, 8, 0, 64, 64, 3, 1, 1, 1, 0), (1, 8, 8, 0, 64, 3, 1, 1, 1, 0),
                (1, 8, 8, 64, 0, 3, 1, 1, 1, 0), (1, 8, 8, 64, 64, 9, 1, 1, 4, 0), (1, 8, 8, 64, 64, 0, 1, 1, 0, 0), (1, 8, 8, 64, 21, 6, 3, 1, 2, 0),
                (1, 8, 8, 64, 32, 4, 2, 2, 1, 0), (1, 8, 8, 64, 64, 3, 1, 0, 1, 0), (1, 8, 8, 64, 64, 7, 1, 12, 36, 0), (1, 8, 8, 64, 64, 3, 1, 5, 5, 0),
                (1, 8, 8, 512, 2, 256, 128, 1, 64, 0), (1, 8, 8, 64, 64, 5, 2, 1, 2, 0)]
    tr_bad = [(0, 8, 8, 16, 64, 8, 4, 2, 0), (1, 8, 8, 0, 64, 8, 4, 2, 0), (1, 8, 8, 16, 64, 6, 4, 2, 0), (1, 8, 8, 16, 48, 6, 3, 1, 0),
              (1, 8, 8, 16, 64, 8, 4, -1, 0), (1, 8, 8, 16, 2048, 256, 128, 64, 0)]
    pl_bad = [(0, 256, 64, 260, 260, 7, 1, 3, 0, 0), (1, 256, 64, 260, 0, 7, 1, 3, 0, 0), (1, 256, 64, 260, 260, 4, 1, 1, 0, 0),
              (1, 256, 64, 260, 260, 8, 1, 3, 0, 0), (1, 256, 64, 260, 260, 7, 0, 3, 0, 0), (1, 256, 64, 260, 260, 7, 11, 33, 0, 0)]
    calls = []
    for ints in conv_bad:
        calls.append(("sat_conv1d_bf16x3", 13, ints, (None,)))
        calls.append(("sat_conv1d_bf16x3_emit", 13, ints, (None, None, None, None, 0, None)))
        calls.append(("sat_conv1d_bf16x3_ws", 13, ints, (None, None, None, None, 0, None, 0, -1, None)))
    calls.append(("sat_conv1d_bf16x3_emit", 13, (1, 8, 8, 64, 64, 3, 1, 1, 1, 0), (None, None, None, None, 0, None)))        # legal shape, no planes
    for n in (5, 17, 65, 1000):       # 16 chunks: a count that leaves a split empty, more splits than chunks, more than SAT_SPLIT_MAX
        calls.append(("sat_conv1d_bf16x3_ws", 13, (2, 256, 32, 136, 136, 3, 1, 1, 1, 0), (None, None, None, None, 0, None, 0, n, None)))
        calls.append(("sat_convtr1d_bf16x3_ws", 13, (2, 512, 32, 68, 136, 4, 2, 1, 0), (None, 0, n, None)))
    calls.append(("sat_conv1d_bf16x3_ws", 13, (2, 256, 64, 260, 260, 7, 1, 1, 3, 0), (None, None, None, None, 0, None, 0, 2, None)))      # the direct k7 kernel
    calls.append(("sat_conv1d_bf16x3_ws", 13, (2, 256, 32, 136, 136, 3, 1, 1, 1, 0), (None, None, None, None, 0, None, 0, 2, None)))      # legal split, no workspace
    calls.append(("sat_convtr1d_bf16x3_ws", 13, (2, 512, 32, 68, 136, 4, 2, 1, 0), (None, 0, 2, None)))
    for ints in tr_bad:
        calls.append(("sat_convtr1d_bf16x3", 13, ints, (None,)))
        calls.append(("sat_convtr1d_bf16x3_ws", 13, ints, (None, 0, -1, None)))
    for ints in pl_bad:
        calls.append(("sat_conv1d_bf16x3_planesq", None, (rows7, *ints), (None,)))
        calls.append(("sat_conv1d_bf16x3_planesq_ws", None, (rows7, *ints), (None, 0, -1, None)))
    calls.append(("sat_conv1d_bf16x3_planesq", None, (rows7 - 1, 1, 256, 64, 260, 260, 7, 1, 3, 0, 0), (None,)))
    calls.append(("sat_conv1d_bf16x3_planesq_ws", None, (rows7 - 1, 1, 256, 64, 260, 260, 7, 1, 3, 0, 0), (None, 0, -1, None)))
    rows_u = lib.sat_conv1d_k7_plane_rows(128, 128, 9)
    for ints in ((0, 64, 128, 7, 3, 9), (1, 0, 128, 7, 3, 9), (1, 64, 0, 7, 3, 9), (1, 129, 128, 7, 3, 9), (1, 64, 128, 4, 1, 1), (1, 64, 128, 8, 2, 7),
                 (1, 64, 128, 7, 0, 0), (1, 64, 128, 7, 11, 33), (1, 64, 128, 7, 3, 8)):
        calls.append(("sat_residual_unit_fwd", None, (rows_u, *ints), (None, None, None, None, 0, None)))
    calls.append(("sat_residual_unit_fwd", None, (rows_u - 1, 1, 64, 128, 7, 3, 9), (None, None, None, None, 0, None)))
    calls.append(("sat_residual_unit_fwd", None, (rows_u, 1, 64, 128, 7, 3, 9), (None, None, None, None, 0, None)))          # legal shape, no operands
    return calls


def call_refusal(lib, name, nptr, ints, tail):
    """-> (status, error text after the entry point's name).  The planes entry points take (planes hi, lo, rows, pointers ..., ints ...)."""
    null = ctypes.c_void_p(None)
    tail = [null if t is None else t for t in tail]
    if nptr is None:
        lead = {"sat_residual_unit_fwd": 11}.get(name, 10)
        args = [null, null, ints[0]] + [null] * lead + list(ints[1:]) + tail
    else:
        args = [null] * nptr + list(ints) + tail
    status = getattr(lib, name)(*args)
    return status, lib.sat_last_error().decode().split(": ", 1)[1]


def tables(lib):
    shapes = sorted(set(flagship_shapes() + edge_shapes()))
    t = {"generator": "tools/gen_golden_conv_host.py", "cus": CUS, "splits": list(SPLITS), "split": []}
    for sh in shapes:
        row = []
        for want in SPLITS:
            need = ctypes.c_longlong(-7)
            n = lib.sat_conv_bf16x3_split(*sh, want, CUS, ctypes.byref(need))
            row.append([n, need.value])
        t["split"].append([list(sh), row])
    t["conv_rows"] = [[b, tout, k, s, lib.sat_conv1d_bf16x3_partial_rows(b, tout, k, s)]
                      for b in (0,) + BS for tout in (0,) + TOUTS + (2097152,) for k in KS + (16, 32, 128, 256) for s in STRIDES]
    t["convtr_rows"] = [[b, tout, s, pad, lib.sat_convtr1d_bf16x3_partial_rows(b, tout, s, pad)]
                        for b in (0,) + BS for tout in (0,) + TOUTS + (2097152,) for s in (0,) + STRIDES for pad in (-1, 0, 1, 4, 64)]
    t["plane_rows"] = [[tin, tout, pad, lib.sat_conv1d_k7_plane_rows(tin, tout, pad)]
                       for tin in (0,) + TOUTS + (1024, 2097152) for tout in (0,) + TOUTS + (1024, 2097152) for pad in (-1, 0, 3, 9, 27, 32, 33)]
    t["pack_size"] = [[d0, d1, k, s, mode, lib.sat_pack_weights_bf16x3_size(d0, d1, k, s, mode)]
                      for d0, d1 in ((0, 8), (8, 0), (1, 2), (129, 65), (64, 128)) for k in KS + (16, 128, 256) for s in STRIDES for mode in (-1, 0, 1, 2, 3)]
    t["pack_k7q_size"] = [[d0, d1, k, mode, lib.sat_pack_weights_k7q_size(d0, d1, k, mode)]
                          for d0 in (0, 1, 64, 129, 2048) for d1 in (0, 2, 65, 128) for k in KS for mode in (-1, 0, 1, 2)]
    t["refusals"] = []
    for name, nptr, ints, tail in refusal_calls(lib):
        status, text = call_refusal(lib, name, nptr, ints, tail)
        assert status != 0, (name, ints, tail)
        t["refusals"].append([name, nptr, list(ints), list(tail), status, text])
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=_lib.LIB_PATH, help="the library whose answers are recorded (default: this tree's gfx950 build)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    t = tables(_lib.bind(ctypes.CDLL(a.lib)))
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in t.items()) + "\n}\n")
    print(f"{os.path.relpath(a.out, ROOT)}: {os.path.getsize(a.out)} bytes; " + ", ".join(f"{k} {len(v)}" for k, v in t.items() if isinstance(v, list)))


if __name__ == "__main__":
    main()
