#!/usr/bin/env python3
"""Project real actions into a trained generator's W space (project.Projector): which latent reproduces this
motion, and how well?

Real data is read through Feeder(norm=True); the first --per_class samples of every class are selected as mmd_actions.py selects
them and cropped to --t_size frames.  Every sample is inverted by --steps iterations of a per-sample Adam on the weighted sum of
a position, a velocity and a bone-length term (--lambdas).  Printed: the class means of the three terms at each sample's best
step (recon_pos, recon_vel, recon_bone; smaller is better).  Written to --out: proj_w.npy (K * per_class, D) the latents,
proj_data.npy the reconstructions in generate.py's layout (NTU: with the trailing person axis), proj_loss.npy (K * per_class, 4) =
[L, L_pos, L_vel, L_bone] and proj_label.pkl, so the other tools take the reconstructions as a generated set.

Completion: --mask_joints 5 6 7 and / or --mask_frames 20:40 give those entries weight 0 (both given: the listed joints inside
the frame range); the objective does not see them.  held_out_pos, the mean squared error of the reconstruction on exactly these
entries, is computed on the host and printed.

    python tools/project_actions.py --model runs/kinetic-gan/models/generator_100000.pth --data_real val_data.npy \\
        --labels_real val_label.pkl --dataset ntu --t_size 64 --per_class 10 --steps 200 --out runs/project"""
import argparse
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kinetic_gan_amd  # noqa: F401,E402
from kinetic_gan_amd.feeder import Feeder  # noqa: E402
from kinetic_gan_amd.generator import Generator  # noqa: E402
from kinetic_gan_amd.metrics import RECON_NAMES, reconstruction, select_reference_samples  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--model", type=str, required=True, help="path to gen model (generator_<n>.pth)")
    p.add_argument("--data_real", type=str, required=True, help="path to real data")
    p.add_argument("--labels_real", type=str, required=True, help="path to real labels")
    p.add_argument("--dataset", type=str, default="ntu", help="dataset")
    p.add_argument("--latent_dim", type=int, default=512, help="dimensionality of the latent space")
    p.add_argument("--mlp_dim", type=int, default=4, help="mapping network depth")
    p.add_argument("--n_classes", type=int, default=None, help="number of classes (default: 60, h36m: 10)")
    p.add_argument("--channels", type=int, default=None, help="number of channels (default: 3, h36m: 2)")
    p.add_argument("--t_size", type=int, default=64, help="Temporal dimension")
    p.add_argument("--per_class", type=int, default=10, help="samples of every class")
    p.add_argument("--batch", type=int, default=64, help="samples per projection batch")
    p.add_argument("--steps", type=int, default=200, help="iterations per batch")
    p.add_argument("--lr", type=float, default=0.05)
    p.add_argument("--lambdas", type=float, nargs=3, default=(1.0, 1.0, 0.1), help="weights of the position, velocity, bone terms")
    p.add_argument("--lambda_w", type=float, default=0.0, help="weight of the prior towards the class mean in W")
    p.add_argument("--noise", type=str, default="zero", choices=["zero", "fixed"], help="the injected noise planes")
    p.add_argument("--mean_size", type=int, default=1000, help="Samples to estimate the class means in W")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--mask_joints", type=int, nargs="*", default=None, help="joints the objective does not see")
    p.add_argument("--mask_frames", type=str, default=None, help="a:b - frames the objective does not see")
    p.add_argument("--out", type=str, default="runs/project", help="output directory")
    p.add_argument("--no-graph", action="store_true", help="run the iterations eagerly instead of replaying a hipGraph")
    return p.parse_args(argv)


def completion_mask(T, V, joints, frames):
    """(T, V) weights: 0 on the masked entries, None when nothing is masked"""
    if not joints and frames is None:
        return None
    a, b = (0, T) if frames is None else (int(v) for v in frames.split(":"))
    if not (0 <= a < b <= T):
        raise SystemExit("--mask_frames %s is not a range inside [0, %d]" % (frames, T))
    js = list(range(V)) if not joints else [int(j) for j in joints]
    if any(not (0 <= j < V) for j in js):
        raise SystemExit("--mask_joints names a joint outside [0, %d)" % V)
    m = np.ones((T, V), dtype=np.float32)
    m[a:b, js] = 0.0
    return m


def main(argv=None):
    opt = parse_args(argv)
    print(opt)
    if not torch.cuda.is_available():
        raise SystemExit("tools/project_actions.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    h36m = opt.dataset == "h36m"
    K = opt.n_classes if opt.n_classes is not None else (10 if h36m else 60)
    C = opt.channels if opt.channels is not None else (2 if h36m else 3)
    G = Generator(opt.latent_dim, C, K, opt.t_size, mlp_dim=opt.mlp_dim, dataset=opt.dataset).to(dev)
    G.load_state_dict(torch.load(opt.model, map_location=dev), strict=False)

    feeder = Feeder(opt.data_real, opt.labels_real, norm=True, dataset=opt.dataset)      # normalised to [-1, 1]
    real, lab, _ = select_reference_samples(feeder, np.arange(K), opt.t_size, opt.per_class)
    print(real.shape, "real")
    T, V = real.shape[2], real.shape[3]
    mask = completion_mask(T, V, opt.mask_joints, opt.mask_frames)
    out = reconstruction(G, torch.from_numpy(real).to(dev), lab, dataset="h36m" if h36m else "ntu", per_class=opt.per_class,
                         mask=mask, n=min(opt.batch, real.shape[0]), steps=opt.steps, lr=opt.lr, lambdas=tuple(opt.lambdas),
                         lambda_w=opt.lambda_w, noise=opt.noise, seed=opt.seed, mean_size=opt.mean_size, use_graph=not opt.no_graph)
    loss = out["per_sample"].reshape(-1, 4).cpu().numpy()
    w = out["best_w"].reshape(loss.shape[0], -1).cpu().numpy()
    recon = out["recon"].reshape((loss.shape[0],) + real.shape[1:]).cpu().numpy()
    frozen = int((out["nonfinite"] > 0).sum())
    if frozen:
        print("samples with a non-finite objective or gradient at some step: %d" % frozen)

    os.makedirs(opt.out, exist_ok=True)
    np.save(os.path.join(opt.out, "proj_w.npy"), w)
    np.save(os.path.join(opt.out, "proj_data.npy"), np.expand_dims(recon, -1) if not h36m else recon)
    np.save(os.path.join(opt.out, "proj_loss.npy"), loss)
    with open(os.path.join(opt.out, "proj_label.pkl"), "wb") as f:
        pickle.dump(np.stack([lab, lab]), f)
    # the printed class means are the means of the written array (float64 on the host)
    res = dict(zip(RECON_NAMES, loss.reshape(K, opt.per_class, 4)[:, :, 1:].astype(np.float64).mean(1).mean(0).tolist()))
    if mask is not None:
        hidden = np.broadcast_to(mask == 0, recon.shape)
        res["held_out_pos"] = float(((recon.astype(np.float64) - real.astype(np.float64)) ** 2)[hidden].mean())
    print(" ".join("%s %.6g" % kv for kv in res.items()))
    print(os.path.join(opt.out, "proj_data.npy"))
    return res


if __name__ == "__main__":
    main()
