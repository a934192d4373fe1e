"""The two launches of the dithered-FSQ bottleneck (csrc/fsq.hip: ops.fsq_encode, ops.fsq_decode_tokens) beside a torch restatement of the
reference's eval quantiser, and beside torch.clone() of the same number of bytes.  HIP events throughout; one JSON line per figure.
    python tools/fsq_bench.py
Shapes (B, C, T), levels [17] * 6, one codebook: the codec-like (16, 6, 1500) — 16 items of 1500 latent frames — and (1, 6, 1048576).
"torch" is what the reference runs in eval mode, written out here on the same (B, C, T) input: transpose to (B, T, C), tanh, add, divide,
round, multiply, subtract, the int64 weighted sum over the digits, transpose back (encode); floor-divide, modulo, multiply, subtract,
transpose (decode).  Per line: six alternated rounds of (fused, torch, clone), each round a HIP graph of 10 calls replayed `reps` times, so
the host's dispatch is not in the figure; "eager_us" is the same call issued 200 times from Python without a graph (dispatch included).
Bytes of a call = bytes read + bytes written (encode: 4 BCT + 4 BCT + 8 BTQ; decode: 8 BTQ + 4 BCT); a clone of n bytes moves 2 n.
profiles/taae/README.md records 5.0 - 5.4 TB/s for the junction kernels and for torch.clone() at 512 MB; COPY_TBPS is its lower figure."""
import json
import sys

import torch

sys.path.insert(0, '.')
from stable_audio_tools_amd.ops import get_ops

COPY_TBPS = 5.0
LEVELS, Q = [17] * 6, 1
o = get_ops()
torch.manual_seed(0)
half_l = 1.0 * 2 / (torch.tensor(LEVELS, dtype=torch.int64) - 1)
levels_t = torch.tensor(LEVELS, dtype=torch.int64)
basis_t = torch.cumprod(torch.tensor([1] + LEVELS[:-1]), dim=0, dtype=torch.int64)


def torch_encode(x):
    b, c, t = x.shape
    z = torch.tanh(x.transpose(1, 2).reshape(b, t, Q, c // Q))
    r = ((z + 1.0) / half_l).round()
    codes = r * half_l - 1.0
    idx = ((((codes + 1.0) / half_l).round().to(torch.int64)) * basis_t).sum(dim=-1)      # the reference re-derives the levels from the codes
    return codes.reshape(b, t, c).transpose(1, 2).contiguous(), idx


def torch_decode(tokens):
    b, t, q = tokens.shape
    lev = (tokens[..., None] // basis_t) % levels_t
    return (lev * half_l - 1.0).reshape(b, t, q * len(LEVELS)).transpose(1, 2).contiguous()


def graph_of(f, calls=10):
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        f()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=st):
            for _ in range(calls):
                f()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g, calls, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (calls * reps) * 1e3


def eager_us(f, n=200):
    for _ in range(10):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    global half_l, levels_t, basis_t
    half_l, levels_t, basis_t = half_l.cuda(), levels_t.cuda(), basis_t.cuda()
    calls = 10
    for (b, c, t) in ((16, 6, 1500), (1, 6, 1048576)):
        reps = 20 if b * c * t > 2 ** 22 else 200
        x = 1.5 * torch.randn(b, c, t, device="cuda")
        codes, tokens = o.fsq_encode(x, LEVELS, Q)
        want_codes, want_tokens = torch_encode(x)
        differ = float((tokens != want_tokens).sum()) / tokens.numel()
        assert differ < 1e-2 and torch.equal(o.fsq_decode_tokens(tokens, LEVELS), codes) and torch.equal(torch_decode(tokens), codes), differ
        ops = {"fsq_encode": (lambda: o.fsq_encode(x, LEVELS, Q), lambda: torch_encode(x), 8 * x.numel() + 8 * tokens.numel()),
               "fsq_decode_tokens": (lambda: o.fsq_decode_tokens(tokens, LEVELS), lambda: torch_decode(tokens), 8 * tokens.numel() + 4 * x.numel())}
        for name, (fused, plain, nbytes) in ops.items():
            blob = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            kinds = {"fused": graph_of(fused, calls), "torch": graph_of(plain, calls), "clone": graph_of(blob.clone, calls)}
            runs = {k: [] for k in kinds}
            for _ in range(6):      # alternate: same process, same box
                for k, g in kinds.items():
                    runs[k].append(round(replay_us(g, calls, reps), 2))
            eager = {"fused": round(eager_us(fused), 2), "torch": round(eager_us(plain), 2)}
            for k in kinds:
                print(json.dumps({"op": name, "shape": [b, c, t], "levels": LEVELS, "launch": k, "us_runs": runs[k], "us_min": min(runs[k]),
                                  "us_max": max(runs[k]), "eager_us": eager.get(k), "bytes": nbytes, "GBps_best": round(nbytes / min(runs[k]) * 1e-3, 1),
                                  "share_of_copy_bandwidth": round(nbytes / min(runs[k]) * 1e-6 / COPY_TBPS, 4)}), flush=True)
            print(json.dumps({"op": name, "shape": [b, c, t], "tokens_differing_from_torch": differ,
                              "fused_over_torch_time_median": round(sorted(runs["fused"])[3] / sorted(runs["torch"])[3], 4),
                              "fused_over_clone_time_best": round(min(runs["fused"]) / min(runs["clone"]), 4),
                              "run_to_run_spread": round(max((max(r) - min(r)) / min(r) for r in runs.values()), 4)}), flush=True)
            del kinds, blob
        del x, codes, tokens
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("tools/fsq_bench.py measures on the GPU; there is none here")
    main()
