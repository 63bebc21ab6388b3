"""Launch times of the chunked continuous / categorical head entries on the device (DESIGN.md,
"Action chunks, pad mask and decoding"): at B = 512, h = 4, A = 8, N = 256,
  * mmt_head_continuous (mse and l1, with a ~70 % pad mask: its three launches) beside
    mmt_action_head kind 0 at h = 1;
  * mmt_head_categorical (masked: three launches) beside mmt_action_head kind 1 at h = 1;
  * mmt_head_categorical_decode, argmax and sampling.
HIP events around `inner` back-to-back calls on the current stream, warm-up first, the entries
alternated inside one repetition, median and min-max of the repetitions. Needs an MI355X."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from multi_modal_transformers_tokenmerge_amd import _C
from multi_modal_transformers_tokenmerge_amd.action_heads.categorical import bin_values
from tools.sampler_bench import summary, time_alternating


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--horizon", type=int, default=4)
    ap.add_argument("--action-dim", type=int, default=8)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("heads_bench needs an MI355X: no device found")
    dev = torch.device("cuda:0")
    B, h, A, N, m = args.batch, args.horizon, args.action_dim, args.bins, 5.0
    W, R = h * A, B * h * A
    s = _C.stream_ptr()
    z = torch.randn((B, W), device=dev) * 3
    y = torch.randn((B, W), device=dev)
    mask = (torch.rand((B, W), device=dev) < 0.7).to(torch.uint8)
    zl = torch.randn((R, N), device=dev) * 3
    edges = torch.from_numpy(np.linspace(-m, m, N + 1, dtype=np.float32)).to(dev)
    values = torch.from_numpy(bin_values((-m, m), N)).to(dev)
    loss = torch.zeros(1, device=dev)
    scratch = torch.empty(R + 1, device=dev)
    dz = torch.empty((B, W), dtype=torch.bfloat16, device=dev)
    dzl = torch.empty((R, N), dtype=torch.bfloat16, device=dev)
    cls = torch.empty(R, dtype=torch.int32, device=dev)
    act = torch.empty(R, device=dev)
    rng = torch.tensor([7, 1], dtype=torch.int32, device=dev)

    def cont(kind):
        return lambda: _C.call("mmt_head_continuous", _C.ptr(z), W, B, h, A, _C.ptr(y),
                               _C.ptr(mask), kind, m, None, _C.ptr(scratch), _C.ptr(loss),
                               _C.ptr(dz), s)

    def dec(mode):
        return lambda: _C.call("mmt_head_categorical_decode", _C.ptr(zl), N, R, N, h * A,
                               _C.ptr(values), mode, 1.0, _C.ptr(rng), 0, _C.ptr(cls), _C.ptr(act), s)

    fns = {
        "action_head kind 0 (h=1)": lambda: _C.call(
            "mmt_action_head", 0, _C.ptr(z), W, B, A, _C.ptr(y), None, 0, m, 1.0 / B, None,
            _C.ptr(loss), _C.ptr(dz), s),
        "head_continuous mse": cont(_C.HEAD_LOSS_MSE),
        "head_continuous l1": cont(_C.HEAD_LOSS_L1),
        "action_head kind 1 (h=1)": lambda: _C.call(
            "mmt_action_head", 1, _C.ptr(zl), N, B * A, N, _C.ptr(y), _C.ptr(edges), N + 1, m,
            1.0 / (B * A), None, _C.ptr(loss), _C.ptr(dzl), s),
        "head_categorical": lambda: _C.call(
            "mmt_head_categorical", _C.ptr(zl), N, R, N, _C.ptr(y), _C.ptr(mask), _C.ptr(edges),
            N + 1, _C.ptr(scratch), _C.ptr(loss), _C.ptr(dzl), _C.ptr(cls), s),
        "decode argmax": dec(_C.DECODE_ARGMAX),
        "decode sample": dec(_C.DECODE_SAMPLE),
    }
    times = time_alternating(fns, args.warmup, args.reps, args.inner)
    rows = [dict(entry=k, B=B, h=h, A=A, N=N, **summary(v)) for k, v in times.items()]
    for row in rows:
        print(json.dumps(row), flush=True)
    _C.call("mmt_device_status", s)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
