#!/usr/bin/env python3
"""Mean, vote, entropy and mutual-information maps of the first n images of a LIDC test split (or the synthetic stand-in of
params_eval_synthetic.yml), S samples each, written to one .npz (DenoisingModel.predict_multiple).

    python tools/uncertainty_maps.py [--params params_eval_synthetic.yml] [--n 8] [--batch 8] [--evaluations S] [--voting majority]
                                     [--t 10025] [--batched] [--synthetic-weights SEED] [--out uncertainty_maps.npz]

S and the voting strategy default to the params file's `evaluations` (largest entry of a list) and `evaluation_vote_strategy`.
Weights: `load_from` of the params file if set, else make_synthetic_state_dict(--synthetic-weights).  Arrays in the file:
image [n,C,H,W], mean [n,K,H,W] fp32, vote [n,H,W] uint8, entropy and mutual_info [n,H,W] fp32 (nats).  Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ccdm_stochastic_segmentation_amd import evaluation as E  # noqa: E402
from ccdm_stochastic_segmentation_amd.unet_spec import make_synthetic_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", default="params_eval_synthetic.yml")
    ap.add_argument("--n", type=int, default=8, help="first n images of the split")
    ap.add_argument("--batch", type=int, default=8, help="images per predict_multiple call")
    ap.add_argument("--evaluations", type=int, default=None, help="samples per image (default: the params file)")
    ap.add_argument("--voting", choices=E.VOTE_STRATEGIES, default=None)
    ap.add_argument("--t", type=int, default=None, help="init_t as the sampler takes it (10000 + k: a strided walk of k steps)")
    ap.add_argument("--batched", action="store_true", help="one sampling call of batch*S samples per batch")
    ap.add_argument("--synthetic-weights", type=int, default=0)
    ap.add_argument("--out", default="uncertainty_maps.npz")
    args = ap.parse_args()
    with open(args.params) as fh:
        params = yaml.safe_load(fh)
    params["dataset_val_max_size"] = args.n
    S, voting = E.vote_settings(params)
    S = args.evaluations or S
    voting = args.voting or voting
    dev = torch.device("cuda:0")
    dataset = E.make_dataset(params)
    image0, labels0, _ = dataset[0]
    model = E.build_from_params(params, [tuple(image0.shape), tuple(labels0.shape[1:])], dev)
    if params.get("load_from"):
        E.load_checkpoint(model, E.expanduservars(params["load_from"]))
    else:
        model.unet.load_state_dict({k: torch.from_numpy(v) for k, v in make_synthetic_state_dict(model.unet.spec, args.synthetic_weights).items()})
    E.apply_sampler_options(model, params)
    n = min(args.n, len(dataset))
    images = torch.stack([dataset[i][0] for i in range(n)])
    t = None if args.t is None else torch.as_tensor(args.t)
    keys = ("mean", "vote", "entropy", "mutual_info")
    out = {k: [] for k in keys}
    t0 = time.perf_counter()
    for b0 in range(0, n, args.batch):
        img = images[b0:b0 + args.batch].to(dev)
        res = model.predict_multiple(img, num_evaluations=S, voting=voting, t=t, batched=args.batched, maps=keys)
        for k in keys:
            v = res[k].cpu()
            out[k].append((v.to(torch.uint8) if k == "vote" else v).numpy())
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    arrays = {k: np.concatenate(v) for k, v in out.items()}
    np.savez_compressed(args.out, image=images.numpy(), S=np.int64(S), voting=np.array(voting), **arrays)
    print(f"{n} images x {S} samples ({voting}{', batched' if args.batched else ''}) in {dt:.2f} s -> {args.out}; "
          f"mean entropy {arrays['entropy'].mean():.4f} nats, mean mutual information {arrays['mutual_info'].mean():.4f} nats")


if __name__ == "__main__":
    main()
