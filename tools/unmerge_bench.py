"""The unmerge kernels in isolation, against the torch forms a user would otherwise write and
against the existing merge backward (the same structure: a row gather streamed in 16-B chunks).

Shape: B = 512 samples, one token set of t0 = 256 patches merged to tf = 64 rows, D = 384, in fp32
and bf16 (OCTO-small after twelve r = 16 blocks).

  unmerge_fwd   mmt_tome_unmerge_fwd            vs torch.take_along_dim on the same tensors
  unmerge_bwd   mmt_tome_unmerge_bwd            vs zeros + Tensor.index_add_ (atomic scatter-add)
  merge_bwd     mmt_tome_merge_wavg_bwd at t = 214, r = 107 (107 rows read, 214 written: 321 rows
                per sample against the unmerge's 320)

Algorithmic HBM bytes per sample (es = element size): unmerge fwd tf*D*es read + t0*D*es written +
4*t0 (the map); unmerge bwd t0*D*es + tf*D*es + 4*(t0 + tf + 1) (members, group_start); merge bwd
(t - r)*D*es + t*D*es + 4*t (pos_map) + 4*(2t - r) (sizes). The torch forms are charged the same
bytes as the kernel they stand in for (their own index traffic is larger).

Times: every variant is captured in its own HIP graph of REPS launches; the graphs are replayed
interleaved, ROUNDS times, each replay between two HIP events; median, min and max over rounds.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from multi_modal_transformers_tokenmerge_amd import _kernels as K

HBM_GBS = 8000.0
REPS, ROUNDS = 10, 15
B, T0, TF, D = 512, 256, 64, 384
MT, MR = 214, 107


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


def variants(dtype, dev):
    es = 2 if dtype == torch.bfloat16 else 4
    gen = torch.Generator(device="cpu").manual_seed(1)
    # a real map: twelve r = 16 merges of random metrics
    source, t = torch.empty((B, T0), dtype=torch.int32, device=dev), T0
    for k in range(12):
        unm, src, dst = K.tome_match(torch.randn((B, t, 64), generator=gen).to(dev), 16)
        K.tome_source_step(K.tome_pos_map(unm, src, dst, t, 16), 16, source, first=(k == 0))
        t -= 16
    gs, members = K.tome_source_groups(source, TF)
    x = torch.randn((B, TF, D), generator=gen).to(dtype).to(dev)
    g = torch.randn((B, T0, D), generator=gen).to(dtype).to(dev)
    out = torch.empty((B, T0, D), dtype=dtype, device=dev)
    gx = torch.empty((B, TF, D), dtype=dtype, device=dev)
    idx = source.long()[..., None].expand(-1, -1, D)
    flat = (source.long() + torch.arange(B, device=dev)[:, None] * TF).view(-1)
    gx_t = torch.empty((B * TF, D), dtype=dtype, device=dev)
    # the merge backward at the same number of rows moved
    unm, src, dst = K.tome_match(torch.randn((B, MT, 64), generator=gen).to(dev), MR)
    xm = torch.randn((B, MT, D), generator=gen).to(dtype).to(dev)
    size = torch.rand((B, MT), generator=gen).add_(1).to(dev)
    xo, so, pm = K.tome_merge_fwd(xm, 0, MT, MR, unm, src, dst, size_in=size)
    go = torch.randn_like(xo)
    gi = torch.empty_like(xm)
    K.device_status()
    # the new kernels compute what the torch forms compute
    ref = torch.take_along_dim(x, idx, 1)
    assert torch.equal(K.tome_unmerge_fwd(x, 0, TF, source, out=out), ref)
    b_fwd = B * ((TF + T0) * D * es + 4 * T0)
    b_bwd = B * ((TF + T0) * D * es + 4 * (T0 + TF + 1))
    b_mrg = B * ((2 * MT - MR) * D * es + 4 * MT + 4 * (2 * MT - MR))

    def torch_bwd():
        gx_t.zero_()
        gx_t.index_add_(0, flat, g.view(B * T0, D))
    return [
        ("unmerge_fwd", b_fwd, lambda: K.tome_unmerge_fwd(x, 0, TF, source, out=out)),
        ("torch.take_along_dim", b_fwd, lambda: torch.take_along_dim(x, idx, 1, out=out)),
        ("unmerge_bwd", b_bwd, lambda: K.tome_unmerge_bwd(g, 0, TF, gs, members, out=gx)),
        ("torch.index_add_", b_bwd, torch_bwd),
        ("merge_wavg_bwd", b_mrg, lambda: K.tome_merge_bwd(go, 0, MT, MR, pm, size, so, out=gi)),
    ]


def main():
    dev = torch.device("cuda")
    for dtype in (torch.float32, torch.bfloat16):
        vs = [(name, byts, capture(fn)) for name, byts, fn in variants(dtype, dev)]
        times = {name: [] for name, _, _ in vs}
        cur = torch.cuda.current_stream()
        for _ in range(ROUNDS):
            for name, _, g in vs:                       # interleaved: one replay each per round
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(cur)
                g.replay()
                b.record(cur)
                b.synchronize()
                times[name].append(a.elapsed_time(b) / REPS * 1e3)
        for name, byts, _ in vs:
            ts = times[name]
            med = statistics.median(ts)
            print(json.dumps(dict(kernel=name, dtype=str(dtype).split(".")[-1], B=B, t0=T0, tf=TF,
                                  D=D, us_median=round(med, 2), us_min=round(min(ts), 2),
                                  us_max=round(max(ts), 2), bytes=byts,
                                  GBps=round(byts / med / 1e3, 1),
                                  hbm_frac=round(byts / med / 1e3 / HBM_GBS, 3))), flush=True)


if __name__ == "__main__":
    main()
