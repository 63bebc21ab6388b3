"""Diffusion head loss timings on the device ("Multi-draw diffusion loss"): the head's
forward + backward at D = H = 384, A = 32, B = 512,
  * the single-draw path (loss_forward + loss_backward on the concatenated buffer);
  * the multi-draw path (loss_forward_multi + loss_backward) at K = 1, 4, 8, without and with a
    pad mask;
  * the fused launch alone (mmt_diffusion_loss_multi on given P and Q) at the same K.
HIP events around each call on the current stream, warm-up first, the sides alternated inside one
repetition, median and min-max of the repetitions. Needs an MI355X."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from multi_modal_transformers_tokenmerge_amd import _C
from multi_modal_transformers_tokenmerge_amd.action_heads.diffusion import DiffusionActionHead
from multi_modal_transformers_tokenmerge_amd.params import ParamStore
from tools.sampler_bench import summary, time_alternating


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--draws", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--json", default=None, help="also write the rows to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("diffusion_loss_bench needs an MI355X: no device found")
    dev = torch.device("cuda:0")
    B, D, A = args.batch, args.dim, args.width
    store = ParamStore()
    head = DiffusionActionHead.create(store, "diffusion_action_head", D, A, 32)
    store.materialize(dev, seed=0)
    rng = torch.tensor([7, 1], dtype=torch.int32, device=dev)
    e = (torch.randn((B, D), device=dev) * 0.5).to(torch.bfloat16)
    actions = torch.randn((B, A), device=dev)
    mask = torch.rand((B, A), device=dev) < 0.7
    cat = head.new_cat(B, dev)
    head.readout_slot(cat).copy_(e)

    def single():
        _, sv = head.loss_forward(cat, actions, rng, 0)
        head.loss_backward(sv)

    def multi(K, m=None):
        def run():
            _, sv = head.loss_forward_multi(e, actions, rng, 0, K, m)
            head.loss_backward(sv)
        return run

    fns = {"single": single}
    for K in args.draws:
        fns[f"multi_K{K}"] = multi(K)
    fns[f"multi_K{args.draws[-1]}_mask"] = multi(args.draws[-1], mask)
    rows = [dict(job="head fwd+bwd", B=B, D=D, A=A,
                 **{k: summary(v) for k, v in time_alternating(fns, args.warmup, args.reps, 4).items()})]
    print(json.dumps(rows[-1]), flush=True)

    # the fused launch alone
    P, Q = head._split_first_dense(e)
    w1, H, s = head.d1.w.bf16, head.hidden, _C.stream_ptr()
    Kmax = max(args.draws)
    bf = lambda *sh: torch.empty(sh, dtype=torch.bfloat16, device=dev)
    t = torch.empty((Kmax, B), dtype=torch.int32, device=dev)
    noisy, h, dh, dpred, dP = bf(Kmax * B, A), bf(Kmax * B, H), bf(Kmax * B, H), bf(Kmax * B, A), bf(B, H)
    loss = torch.empty(1, device=dev)
    scratch = torch.empty(B + 1, device=dev)
    dQ = torch.empty((32, H), device=dev)

    def launch(K):
        return lambda: _C.call(
            "mmt_diffusion_loss_multi", _C.ptr(rng), B, A, K, 32, H, 0, _C.ptr(actions), None,
            _C.ptr(head.consts(dev)), _C.ptr(P), P.stride(0), _C.ptr(Q), Q.stride(0), _C.ptr(w1),
            w1.stride(0), _C.ptr(head.d2.w.bf16), _C.ptr(head.d2.b.data), None, None, 1.0,
            _C.ptr(scratch), _C.ptr(loss), _C.ptr(t), None, _C.ptr(noisy), _C.ptr(h), _C.ptr(dh),
            _C.ptr(dpred), _C.ptr(dP), s)

    def dq(K):
        return lambda: _C.call("mmt_diffusion_loss_dq", _C.ptr(t), _C.ptr(dh), H, K * B, 32, H,
                               _C.ptr(dQ), H, s)

    fns = {f"loss_K{K}": launch(K) for K in args.draws}
    fns.update({f"dq_K{K}": dq(K) for K in args.draws})
    rows.append(dict(job="launches alone", B=B, D=D, A=A,
                     **{k: summary(v) for k, v in time_alternating(fns, args.warmup, args.reps, 16).items()}))
    print(json.dumps(rows[-1]), flush=True)
    _C.call("mmt_device_status", _C.stream_ptr())
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
