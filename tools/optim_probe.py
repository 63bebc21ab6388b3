"""Timings of the optimizer launches (include/mmt_api.h) on one MI355X:

    python tools/optim_probe.py                    # the three launches at both parameter counts
    python tools/optim_probe.py --step --batch 512 # + the graphed single-GPU train step

* kernels: mmt_adamw (the yardstick), mmt_adamw_dev and mmt_optim_prepare (both of its launches)
  over the flat parameter count of octo_small and ref_octo_base, and the grouped launches
  mmt_adamw_groups / mmt_optim_prepare_groups with three chunk-flag tables of that model: no bit
  set ("none"), AdamW(weight_decay_mask="kernels") and AdamW(frozen_keys="head_only"). HIP
  events around batches of --inner launches, all variants interleaved (in rotating order) over
  --rounds rounds in one process after a warm-up of every variant; per launch: median, min and
  the 10th..90th percentile spread. The buffers (18 B of state + 4 B of gradient per parameter, 0.4 GB at
  22.5 M) exceed the 256 MB Infinity Cache, so the launches stream from HBM as in a training
  step.
* parameter EMA: mmt_adamw_ema (constant decay 0.999) in its three forms, "host" (mmt_adamw's
  arguments), "opt" (mmt_adamw_dev's) and "groups" (mmt_adamw_groups' with the "kernels" table),
  and the unfused alternative, mmt_adamw followed by ``ema.lerp_(p, 1 - d)``; by bytes 38 B per
  parameter against AdamW's 30 B (1.27x), the unfused pair 42 B.
* --yardstick LIB: a second build of the library (e.g. the parent commit's libmmt_hip.so), whose
  mmt_adamw / mmt_adamw_dev / mmt_adamw_groups[none] are timed in the same rotation as
  "yardstick:<name>": the same box, the same process, interleaved.
* --step: ms per step of distributed.DDPStep's one-graph step at the bench configuration with
  the default AdamW(), with a warm-up-cosine schedule + clipping + skip_nonfinite, and with
  AdamW(frozen_keys="head_only") (the backward stops at the heads), the step objects alternating
  in blocks of --step-block steps.

Prints one JSON line. Needs a GPU: there is no fallback.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_modal_transformers_tokenmerge_amd import _C  # noqa: E402
from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config  # noqa: E402
from multi_modal_transformers_tokenmerge_amd.models.octo import octo as O  # noqa: E402
from multi_modal_transformers_tokenmerge_amd.schedules import (ConstantEmaDecay,  # noqa: E402
                                                               WarmupCosine)

HYPER = (0.9, 0.999, 1e-8, 1e-4)
HBM_PEAK_GBS = 8000.0  # MI355X (MI355X_MICROARCH.md, chip table)


GROUP_TABLES = {"none": dict(weight_decay_mask="*"), "kernels": dict(weight_decay_mask="kernels"),
                "head_only": dict(frozen_keys="head_only")}


def flat_count(config: str):
    """Elements of the flat fp32 master buffer (what AdamW runs over) and the chunk-flag tables
    of GROUP_TABLES for that model, from a model built on the CPU."""
    model = O.Octo(get_config(config), torch.device("cpu"), seed=0)
    tables = {}
    for name, kw in GROUP_TABLES.items():
        model.set_param_groups(kw.get("weight_decay_mask"), kw.get("frozen_keys"))
        tables[name] = model.store.chunk_flags.clone()
    return model.store.flat.numel(), tables


def _stats(us):
    a = np.asarray(us)
    return dict(median_us=round(float(np.median(a)), 2), min_us=round(float(a.min()), 2),
                p10_us=round(float(np.percentile(a, 10)), 2),
                p90_us=round(float(np.percentile(a, 90)), 2))


def load_yardstick(path: str):
    """A second build of the C ABI, bound for the three AdamW launches only."""
    h = ctypes.CDLL(os.path.abspath(path))
    for name in ("mmt_adamw", "mmt_adamw_dev", "mmt_adamw_groups"):
        fn = getattr(h, name)
        fn.argtypes, fn.restype = _C.SIGNATURES[name], ctypes.c_int
    return h


def probe_kernels(n: int, tables: dict, dev, rounds: int, inner: int, warm: int,
                  yard=None) -> dict:
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, generator=gen, device=dev)
    g = torch.randn(n, generator=gen, device=dev) * 1e-2
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    shadow = torch.empty(n, dtype=torch.bfloat16, device=dev)
    state = torch.tensor([1234, 0], dtype=torch.int32, device=dev)
    opt = torch.zeros(_C.OPT_WORDS, device=dev)
    ws = torch.empty(_C.workspace_size(_C.WS_GRAD_NORM, n), dtype=torch.uint8, device=dev)
    sched = WarmupCosine(0.0, 3e-4, 2000, 300000, 3e-5).to_c()
    s = _C.stream_ptr()

    def adamw():
        _C.call("mmt_adamw", _C.ptr(p), _C.ptr(g), _C.ptr(m), _C.ptr(v), _C.ptr(shadow), n,
                _C.ptr(state), 3e-4, *HYPER, 1.0, s)

    def adamw_dev():
        _C.call("mmt_adamw_dev", _C.ptr(p), _C.ptr(g), _C.ptr(m), _C.ptr(v), _C.ptr(shadow), n,
                _C.ptr(state), _C.ptr(opt), *HYPER, s)

    def prepare():
        _C.call("mmt_optim_prepare", _C.ptr(g), n, 1.0, 1.0, 1, ctypes.addressof(sched),
                _C.ptr(state), _C.ptr(opt), _C.ptr(ws), ws.numel(), s)

    variants = {"mmt_adamw": adamw, "mmt_adamw_dev": adamw_dev, "mmt_optim_prepare": prepare}
    flags = {k: t.to(dev) for k, t in tables.items()}
    assert all(t.numel() == -(-n // 64) for t in flags.values())

    def adamw_groups(t):
        return lambda: _C.call("mmt_adamw_groups", _C.ptr(p), _C.ptr(g), _C.ptr(m), _C.ptr(v),
                               _C.ptr(shadow), n, _C.ptr(state), None, 3e-4, *HYPER, 1.0,
                               _C.ptr(t), 64, s)

    def prepare_groups(t):
        return lambda: _C.call("mmt_optim_prepare_groups", _C.ptr(g), n, 1.0, 1.0, 1,
                               ctypes.addressof(sched), _C.ptr(state), _C.ptr(opt), _C.ptr(ws),
                               ws.numel(), _C.ptr(t), 64, s)

    for k, t in flags.items():
        variants[f"mmt_adamw_groups[{k}]"] = adamw_groups(t)
        variants[f"mmt_optim_prepare_groups[{k}]"] = prepare_groups(t)

    # parameter EMA: the fused launch in its three forms, and AdamW + a torch pass
    ema = p.clone()
    decay = ConstantEmaDecay(0.999).to_c()

    def adamw_ema(o, t):
        return lambda: _C.call("mmt_adamw_ema", _C.ptr(p), _C.ptr(g), _C.ptr(m), _C.ptr(v),
                               _C.ptr(shadow), _C.ptr(ema), n, _C.ptr(state), _C.ptr(o), 3e-4,
                               *HYPER, 1.0, _C.ptr(t), 64, ctypes.addressof(decay), s)

    def unfused():
        adamw()
        ema.lerp_(p, 1.0 - 0.999)

    variants["mmt_adamw_ema[host]"] = adamw_ema(None, None)
    variants["mmt_adamw_ema[opt]"] = adamw_ema(opt, None)
    variants["mmt_adamw_ema[groups]"] = adamw_ema(None, flags["kernels"])
    variants["mmt_adamw+lerp"] = unfused
    if yard is not None:
        none = flags["none"]
        variants["yardstick:mmt_adamw"] = lambda: yard.mmt_adamw(
            _C.ptr(p), _C.ptr(g), _C.ptr(m), _C.ptr(v), _C.ptr(shadow), n, _C.ptr(state), 3e-4,
            *HYPER, 1.0, s)
        variants["yardstick:mmt_adamw_dev"] = lambda: yard.mmt_adamw_dev(
            _C.ptr(p), _C.ptr(g), _C.ptr(m), _C.ptr(v), _C.ptr(shadow), n, _C.ptr(state),
            _C.ptr(opt), *HYPER, s)
        variants["yardstick:mmt_adamw_groups[none]"] = lambda: yard.mmt_adamw_groups(
            _C.ptr(p), _C.ptr(g), _C.ptr(m), _C.ptr(v), _C.ptr(shadow), n, _C.ptr(state), None,
            3e-4, *HYPER, 1.0, _C.ptr(none), 64, s)
    prepare()  # opt holds a learning rate and a clip factor before the first mmt_adamw_dev
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    names = list(variants)
    for r in range(rounds):
        k = r % len(names)
        for name in names[k:] + names[:k]:  # every variant follows every other one
            fn = variants[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    assert bool(torch.isfinite(p).all()) and float(opt[_C.OPT_SKIPPED]) == 0
    out = {k: _stats(t) for k, t in times.items()}
    base = out["mmt_adamw"]
    out["adamw_spread_rel"] = round((base["p90_us"] - base["p10_us"]) / base["median_us"], 4)
    out["adamw_dev_over_adamw"] = round(out["mmt_adamw_dev"]["median_us"] / base["median_us"], 4)
    out["prepare_over_adamw"] = round(out["mmt_optim_prepare"]["median_us"] / base["median_us"], 4)
    out["adamw_gbs"] = round(30.0 * n / base["median_us"] / 1e3, 1)  # 30 B per parameter
    gbs = 4.0 * n / out["mmt_optim_prepare"]["median_us"] / 1e3      # 4 B per parameter
    out["prepare_gbs"] = round(gbs, 1)
    out["prepare_hbm_fraction"] = round(gbs / HBM_PEAK_GBS, 3)
    prep = out["mmt_optim_prepare"]
    for k in flags:  # the grouped launches against the plain kernel of the same build
        a, q = out[f"mmt_adamw_groups[{k}]"], out[f"mmt_optim_prepare_groups[{k}]"]
        out[f"adamw_groups[{k}]_over_adamw"] = round(a["median_us"] / base["median_us"], 4)
        out[f"prepare_groups[{k}]_over_prepare"] = round(q["median_us"] / prep["median_us"], 4)
    a = out["mmt_adamw_groups[none]"]["median_us"]
    out["adamw_groups[none]_inside_adamw_p10_p90"] = bool(base["p10_us"] <= a <= base["p90_us"])
    q = out["mmt_optim_prepare_groups[none]"]["median_us"]
    out["prepare_groups[none]_inside_prepare_p10_p90"] = bool(prep["p10_us"] <= q <= prep["p90_us"])
    # the EMA launches against the yardstick: the other build's mmt_adamw if one was given, else
    # this build's; accepted up to the byte ratio 38 / 30 plus the yardstick's own spread
    ref = out.get("yardstick:mmt_adamw", base)
    spread = (ref["p90_us"] - ref["p10_us"]) / ref["median_us"]
    out["ema_yardstick"] = "yardstick:mmt_adamw" if yard is not None else "mmt_adamw"
    out["ema_yardstick_spread_rel"] = round(spread, 4)
    out["ema_accept_ratio"] = round(38.0 / 30.0 + spread, 4)
    for k in ("mmt_adamw_ema[host]", "mmt_adamw_ema[opt]", "mmt_adamw_ema[groups]",
              "mmt_adamw+lerp"):
        out[f"{k}_over_yardstick"] = round(out[k]["median_us"] / ref["median_us"], 4)
    out["adamw_ema_gbs"] = round(38.0 * n / out["mmt_adamw_ema[host]"]["median_us"] / 1e3, 1)
    out["adamw_ema_within_byte_ratio"] = bool(
        out["mmt_adamw_ema[host]_over_yardstick"] <= out["ema_accept_ratio"])
    if yard is not None:  # the unchanged entry points against the other build's
        for k in ("mmt_adamw", "mmt_adamw_dev", "mmt_adamw_groups[none]"):
            out[f"{k}_over_yardstick"] = round(
                out[k]["median_us"] / out[f"yardstick:{k}"]["median_us"], 4)
    return out


def probe_step(config: str, B: int, dev, steps: int, block: int, warm: int) -> dict:
    """The one-graph step with the plain and with the device-controlled optimizer: two models
    with the same weights, their graphs replayed alternately in blocks."""
    from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep
    rng = np.random.default_rng(0)
    runs = {}
    for name, tx in (("default", O.AdamW()),
                     ("schedule_clip", O.AdamW(WarmupCosine(0.0, 3e-4, 2000, 300000, 3e-5),
                                               max_grad_norm=1.0, skip_nonfinite=True)),
                     ("head_only", O.AdamW(frozen_keys="head_only"))):
        model = O.Octo(get_config(config), dev, seed=0)
        cfg, H = model.cfg, model.cfg.image_size[0]
        if not runs:
            img = torch.from_numpy(rng.integers(0, 256, (B, model.n_images, H, H, 3),
                                                dtype=np.uint8)).to(dev)
            txt = (torch.from_numpy(rng.integers(0, cfg.t5.vocab_size, (B, model.n_text),
                                                 dtype=np.int32)).to(dev)
                   if model.has_text else None)
            act = torch.from_numpy(rng.uniform(-1, 1, (B, cfg.action_space_dim))
                                   .astype(np.float32)).to(dev)
        state = O.create_octo_train_state(model, tx, seed=1234)
        step = DDPStep(model, state, txt, img, act, None, txt_next=txt).build()
        for _ in range(warm):
            step()
        runs[name] = (step, state, [])
    torch.cuda.synchronize()
    for _ in range(max(1, steps // block)):
        for name, (step, _, ms) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                step()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / block)
    out = {}
    for name, (_, state, ms) in runs.items():
        a = np.asarray(ms)
        out[name] = dict(median_ms=round(float(np.median(a)), 4), min_ms=round(float(a.min()), 4),
                         p10_ms=round(float(np.percentile(a, 10)), 4),
                         p90_ms=round(float(np.percentile(a, 90)), 4))
        if state.opt is not None:
            out[name].update(last_lr=state.last_lr, last_grad_norm=state.last_grad_norm,
                             last_clip=state.last_clip, skipped_steps=state.skipped_steps)
    out["delta_us"] = round((out["schedule_clip"]["median_ms"] - out["default"]["median_ms"]) * 1e3, 1)
    out["head_only_over_default"] = round(out["head_only"]["median_ms"]
                                          / out["default"]["median_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--configs", nargs="*", default=["octo_small", "ref_octo_base"])
    ap.add_argument("--rounds", type=int, default=42)
    ap.add_argument("--inner", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--yardstick", default=None, metavar="LIB",
                    help="a second build of libmmt_hip.so to time in the same rotation")
    ap.add_argument("--step", action="store_true", help="also time the graphed train step")
    ap.add_argument("--step-config", default="octo-small-tome16")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--step-block", type=int, default=10)
    ap.add_argument("--step-warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "optim_probe needs an MI355X"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "inner": args.inner,
           "kernels": {}}
    yard = load_yardstick(args.yardstick) if args.yardstick else None
    for c in args.configs:
        n, tables = flat_count(c)
        res["kernels"][c] = dict(n=n, **probe_kernels(n, tables, dev, args.rounds, args.inner,
                                                      args.warmup, yard))
    if args.step:
        res["step"] = dict(config=args.step_config, batch=args.batch, steps=args.steps,
                           **probe_step(args.step_config, args.batch, dev, args.steps,
                                        args.step_block, args.step_warmup))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
