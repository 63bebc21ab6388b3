"""Step time of the captured training step with the observation pad masks (DESIGN.md,
"Observation pad masks"): bench.py's step (DDPStep, one HIP graph, the T5 of the next step beside
it) at --config / --batch under one of three settings,

  --mode none   no mask: the step bench.py times
  --mode set    set_pad_mask alone, every set present (the biased attention kernels with a zero
                bias, the pack / bias / row kernels)
  --mode both   set_pad_mask and text_pad_mask with the gaps of a data mixture: a quarter of the
                samples without the (last) camera, instructions of 5 .. 10 real tokens

one setting per process; run each with a time limit of its own. Prints one JSON line."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from bench import synthetic_inputs  # noqa: E402
from multi_modal_transformers_tokenmerge_amd import _kernels as K  # noqa: E402
from multi_modal_transformers_tokenmerge_amd.distributed import DDPStep  # noqa: E402
from multi_modal_transformers_tokenmerge_amd.models.octo.config import get_config  # noqa: E402
from multi_modal_transformers_tokenmerge_amd.models.octo.octo import (  # noqa: E402
    Octo, create_octo_train_state)
from multi_modal_transformers_tokenmerge_amd.tokenizers.token_sequencer import Image  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("none", "set", "both"), default="none")
    ap.add_argument("--config", default="octo-small-tome16")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model = Octo(get_config(args.config), dev, seed=0)
    B = args.batch
    state = create_octo_train_state(model, seed=1234)
    txt, img, act = synthetic_inputs(model, B, 0, dev)
    kw = {}
    if args.mode != "none":
        sm = torch.ones((B, model.n_sets), dtype=torch.bool)
        if args.mode == "both":
            cams = [i for i, ts in enumerate(model.seq.token_sequence) if isinstance(ts, Image)]
            sm[::4, cams[-1]] = False
            T = model.seq.token_sequence[model.text_set].num_tokens
            n = torch.from_numpy(np.random.default_rng(0).integers(5, 11, B))
            kw["text_pad_mask"] = (torch.arange(T)[None, :] < n[:, None]).to(dev)
        kw["set_pad_mask"] = sm.to(dev)
    step = DDPStep(model, state, txt, img, act, None, use_graph=True,
                   txt_next=txt if model.has_text else None, **kw).build()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    cur = torch.cuda.current_stream()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    evs[0].record(cur)
    for i in range(args.steps):
        step()
        evs[i + 1].record(cur)
    torch.cuda.synchronize()
    K.device_status()
    ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps)]
    print(json.dumps({"mode": args.mode, "config": args.config, "batch": B, "steps": args.steps,
                      "median_ms_per_step": round(float(np.median(ms)), 3),
                      "p10_p90_ms_per_step": [round(float(np.percentile(ms, 10)), 3),
                                              round(float(np.percentile(ms, 90)), 3)],
                      "samples_per_s": round(B / float(np.median(ms)) * 1e3, 1),
                      "final_loss": round(float(step.loss_buf.item()), 5)}), flush=True)


if __name__ == "__main__":
    main()
