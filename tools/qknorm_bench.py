"""The QK-norm kernels (csrc/qknorm.hip) in isolation at the step's shapes: B = 512 samples,
D = 384, H = 6 (Dh 64), bf16, at L = 292 (block 0 of OCTO-small) and summed over the twelve
lengths 292, 276, ..., 116 of octo-small-tome16.

Forward: mmt_qk_norm_fwd in place on the packed (B L, 3 D) QKV buffer with qk_pre saved (the
training form) and without (evaluation). Backward: mmt_qk_norm_bwd in place on dqkv, its
scale-gradient pass included. Algorithmic bytes per token row: forward read 2 D, write 2 D
normalised, write 2 D saved; backward read 2 D dy, read 2 D saved, write 2 D dx (the V third is
never touched). Times: every variant captured in its own HIP graph of REPS launches, the graphs
replayed interleaved, ROUNDS times, each replay between two HIP events; median, min and max per
launch, and the achieved GB/s against the 8000 GB/s HBM peak.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from multi_modal_transformers_tokenmerge_amd import _kernels as K

REPS, ROUNDS = 10, 21
B, L, D, H = 512, 292, 384, 6
LENGTHS = [292 - 16 * i for i in range(12)]
HBM_PEAK_GBS = 8000.0


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def variants(dev, length):
    Dh = D // H
    g = torch.Generator().manual_seed(length)
    qkv = (torch.randn((B * length, 3 * D), generator=g) + 1.0).to(torch.bfloat16).to(dev)
    dqkv = torch.randn((B * length, 3 * D), generator=g).to(torch.bfloat16).to(dev)
    qs = (torch.rand(Dh, generator=g) + 0.5).to(dev)
    ks = (torch.rand(Dh, generator=g) + 0.5).to(dev)
    dq, dk = torch.zeros(Dh, device=dev), torch.zeros(Dh, device=dev)
    pre = K.qk_norm_fwd(qkv.clone(), H, Dh, qs, ks)
    row = 2 * D * 2   # bytes of the q and k thirds of one token row
    n = B * length
    return {
        "fwd": (lambda: K.qk_norm_fwd(qkv, H, Dh, qs, ks), 3 * row * n),
        "fwd_eval": (lambda: K.qk_norm_fwd(qkv, H, Dh, qs, ks, save=False), 2 * row * n),
        "bwd": (lambda: K.qk_norm_bwd(dqkv, pre, H, Dh, qs, ks, dq, dk), 3 * row * n),
    }


def measure(passes):
    graphs = {name: capture(fn) for name, (fn, _) in passes.items()}
    times = {name: [] for name in passes}
    for _ in range(ROUNDS):
        for name, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / REPS)
    out = {}
    for name, t in times.items():
        med = statistics.median(t)
        gbs = passes[name][1] / med * 1e-3
        out[name] = dict(us_median=round(med, 1), us_min=round(min(t), 1), us_max=round(max(t), 1),
                         bytes=passes[name][1], gb_s=round(gbs, 1),
                         frac_hbm_peak=round(gbs / HBM_PEAK_GBS, 4))
    return out


def main():
    dev = torch.device("cuda:0")
    out = {"shape": dict(B=B, L=L, D=D, H=H, dtype="bf16"), "reps": REPS, "rounds": ROUNDS,
           "hbm_peak_gb_s": HBM_PEAK_GBS}
    out.update(measure(variants(dev, L)))
    total = {"fwd": 0.0, "bwd": 0.0}
    per_len = {}
    for length in LENGTHS:
        passes = variants(dev, length)
        m = measure({k: passes[k] for k in total})
        per_len[length] = {k: m[k]["us_median"] for k in total}
        for k in total:
            total[k] += m[k]["us_median"]
    out["per_length_us"] = per_len
    out["twelve_blocks_us"] = {k: round(v, 1) for k, v in total.items()}
    K.device_status()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
