"""The diffusion head's forward + backward with the readouts averaged (readout_pooling="mean") and
pooled by attention ("attention"), in isolation: B = 512 samples, D = 384, the 4 readout rows of a
100-row final sequence (OCTO-small after twelve r = 16 merges), 6 pooling heads.

Each variant runs readout pooling -> DiffusionActionHead.loss_forward -> loss_backward -> pooling
backward (the whole dxL written), the dW products on the side stream as in the step
(layers.wgrad_overlap). Times: every variant captured in its own HIP graph of REPS passes; the
graphs replayed interleaved, ROUNDS times, each replay between two HIP events; median, min and max
per pass. Launch counts: C-ABI calls (a split-K GEMM is one call, two launches) counted over one
eager pass, and the elementwise torch kernels around the M = 1 query projection.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from multi_modal_transformers_tokenmerge_amd import _C
from multi_modal_transformers_tokenmerge_amd.action_heads.diffusion import DiffusionActionHead
from multi_modal_transformers_tokenmerge_amd.attention_blocks.attention import MultiHeadAttentionPooling
from multi_modal_transformers_tokenmerge_amd.layers import wgrad_overlap
from multi_modal_transformers_tokenmerge_amd.params import ParamStore

REPS, ROUNDS = 10, 21
B, L, D, N, H = 512, 100, 384, 4, 6


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


def main():
    dev = torch.device("cuda:0")
    store = ParamStore()
    head = DiffusionActionHead.create(store, "diffusion_action_head", D)
    pool = MultiHeadAttentionPooling.create(store, "diffusion_action_head/MultiHeadAttentionPooling_0",
                                            D, H)
    store.materialize(dev, 0)
    g = torch.Generator().manual_seed(0)
    xL = torch.randn((B, L, D), generator=g).to(dev)
    actions = (torch.rand((B, 8), generator=g) * 2 - 1).to(dev)
    rng = torch.tensor([1234, 0], dtype=torch.int32, device=dev)
    rows = torch.arange(L - N, L, dtype=torch.int32, device=dev)
    flag = torch.full((L,), -1, dtype=torch.int32)
    flag[L - N:] = torch.arange(N, dtype=torch.int32)
    flag = flag.to(dev)

    def mean_pass():
        cat = head.new_cat(B, dev)
        _C.call("mmt_rows_mean_fwd", _C.ptr(xL), xL.stride(0), xL.stride(1), B, D, _C.ptr(rows), N,
                _C.ptr(head.readout_slot(cat)), cat.stride(0), _C.stream_ptr())
        _, sv = head.loss_forward(cat, actions, rng)
        with wgrad_overlap(dev):
            de = head.loss_backward(sv)
            dx = torch.empty((B, L, D), dtype=torch.float32, device=dev)
            _C.call("mmt_rows_mean_bwd", _C.ptr(de), de.stride(0), B, L, D, _C.ptr(flag), N,
                    _C.ptr(dx), _C.stream_ptr())
        return dx

    def attn_pass():
        cat = head.new_cat(B, dev)
        _, psv = pool.forward(xL, rows, out=head.readout_slot(cat))
        _, sv = head.loss_forward(cat, actions, rng)
        with wgrad_overlap(dev):
            de = head.loss_backward(sv)
            return pool.backward(de, psv, flag)

    passes = {"mean": mean_pass, "attention": attn_pass}
    calls = {}
    real = _C.call
    for name, fn in passes.items():   # C-ABI calls of one eager pass
        n = [0]

        def counting(*a, _n=n, **k):
            _n[0] += 1
            return real(*a, **k)
        _C.call = counting
        try:
            fn()
        finally:
            _C.call = real
        torch.cuda.synchronize()
        calls[name] = n[0]
    graphs = {name: capture(fn) for name, fn in passes.items()}
    times = {name: [] for name in passes}
    for _ in range(ROUNDS):
        for name, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / REPS)
    out = {"shape": dict(B=B, L=L, D=D, n=N, H=H), "reps": REPS, "rounds": ROUNDS}
    for name, t in times.items():
        out[name] = dict(us_median=round(statistics.median(t), 1), us_min=round(min(t), 1),
                         us_max=round(max(t), 1), c_abi_calls=calls[name])
    out["attention"]["torch_elementwise_kernels"] = 8    # 1 forward (query scale), 7 backward
    out["delta_us"] = round(out["attention"]["us_median"] - out["mean"]["us_median"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
