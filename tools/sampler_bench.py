"""Diffusion sampler timings on the device ("Step-table sampler"): at D = H = 384 and
B in {1, 64, 512},
  * the fused step-table sampler (mmt_diffusion_sample_steps behind predict_action_mean) against
    the per-step launch loop (_predict_action_loop), at A = 32 for 32 fresh-noise DDPM steps and
    for DDIM K = 8: whole calls, time-embedding and P / Q GEMMs included on both sides;
  * at A = 8, the step-table kernel on the reference's frozen 32-step table against the legacy
    register-resident kernel (mmt_diffusion_sample): whole calls, and the sampler launch alone.
HIP events around each call on the current stream, warm-up first, the two sides of a comparison
alternated inside one repetition, median and min-max of the repetitions. Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from multi_modal_transformers_tokenmerge_amd import _C
from multi_modal_transformers_tokenmerge_amd.action_heads.diffusion import (DiffusionActionHead,
                                                                            SamplerSpec)
from multi_modal_transformers_tokenmerge_amd.params import ParamStore


def time_alternating(fns: dict, warmup: int, reps: int, inner: int) -> dict:
    """{name: [us per call] * reps}: every repetition times `inner` back-to-back calls of each
    function in turn between two events."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for name, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    return out


def summary(us: list) -> dict:
    return dict(median_us=round(statistics.median(us), 2), min_us=round(min(us), 2),
                max_us=round(max(us), 2))


def make_head(dev, D, A):
    store = ParamStore()
    head = DiffusionActionHead.create(store, "diffusion_action_head", D, A, 32)
    store.materialize(dev, seed=0)
    return head


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 512])
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sampler_bench needs an MI355X: no device found")
    dev = torch.device("cuda:0")
    D = args.dim
    rng = torch.tensor([7, 1], dtype=torch.int32, device=dev)
    rows = []

    def report(job, B, times):
        row = dict(job=job, D=D, B=B, **{k: summary(v) for k, v in times.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)

    wide, narrow = make_head(dev, D, 32), make_head(dev, D, 8)
    for B in args.batches:
        readout = (torch.randn((B, D), device=dev) * 0.5).to(torch.bfloat16)
        for job, spec in (("A32 ddpm32 fresh", SamplerSpec(noise="fresh")),
                          ("A32 ddim8", SamplerSpec("ddim", 8))):
            t = time_alternating(
                {"fused": lambda: wide.predict_action_mean(readout, rng, sampler=spec),
                 "loop": lambda: wide._predict_action_loop(readout, rng, 0, None, False, spec=spec)},
                args.warmup, args.reps, inner=4)
            report(job, B, t)
        # A = 8, the reference's frozen 32-step job: whole calls, then the sampler launch alone
        ref_spec = SamplerSpec()
        t = time_alternating(
            {"legacy": lambda: narrow.predict_action_mean(readout, rng),
             "steps": lambda: narrow._sample_steps(readout, rng, 0, None, None, ref_spec)},
            args.warmup, args.reps, inner=8)
        report("A8 ddpm32 frozen, call", B, t)
        P, Q = narrow._split_first_dense(readout)
        w1, w2, b2 = narrow.d1.w.bf16, narrow.d2.w.bf16, narrow.d2.b.data
        t_dev, coef_dev, _ = narrow._table_dev(ref_spec, dev)
        actions = torch.empty((B, 8), dtype=torch.float32, device=dev)
        s = _C.stream_ptr()
        t = time_alternating(
            {"legacy": lambda: _C.call(
                "mmt_diffusion_sample", _C.ptr(rng), B, 8, 32, 0, _C.ptr(P), P.stride(0),
                _C.ptr(Q), Q.stride(0), _C.ptr(w1), w1.stride(0), _C.ptr(w2), _C.ptr(b2),
                _C.ptr(narrow.sampler_coef(dev)), None, narrow.hidden, _C.ptr(actions), None, s),
             "steps": lambda: _C.call(
                "mmt_diffusion_sample_steps", _C.ptr(rng), B, 8, 32, 0, _C.ptr(P), P.stride(0),
                _C.ptr(Q), Q.stride(0), 32, _C.ptr(w1), w1.stride(0), _C.ptr(w2), _C.ptr(b2),
                _C.ptr(t_dev), _C.ptr(coef_dev), 5.0, 0, None, None, narrow.hidden,
                _C.ptr(actions), None, None, s)},
            args.warmup, args.reps, inner=32)
        report("A8 ddpm32 frozen, launch", B, t)
        # the wide kernel alone, for the kernel's own time at A = 32
        P, Q = wide._split_first_dense(readout)
        w1, w2, b2 = wide.d1.w.bf16, wide.d2.w.bf16, wide.d2.b.data
        act32 = torch.empty((B, 32), dtype=torch.float32, device=dev)
        fns = {}
        for name, spec in (("ddpm32_fresh", SamplerSpec(noise="fresh")), ("ddim8", SamplerSpec("ddim", 8))):
            td, cd, tn = wide._table_dev(spec, dev)
            fns[name] = (lambda td=td, cd=cd, n=len(tn), fl=int(spec.fresh): _C.call(
                "mmt_diffusion_sample_steps", _C.ptr(rng), B, 32, n, 0, _C.ptr(P), P.stride(0),
                _C.ptr(Q), Q.stride(0), 32, _C.ptr(w1), w1.stride(0), _C.ptr(w2), _C.ptr(b2),
                _C.ptr(td), _C.ptr(cd), 5.0, fl, None, None, wide.hidden, _C.ptr(act32), None,
                None, s))
        report("A32, launch", B, time_alternating(fns, args.warmup, args.reps, inner=32))
    _C.call("mmt_device_status", _C.stream_ptr())
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
