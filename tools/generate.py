#!/usr/bin/env python
"""The reference's sampling program (generate.py) on ``kinetic_gan_amd.sample.Sampler``: same flags, same three output
files - ``<n>_<gen_qtd>[_trunc<t>][_stochastic]_gen_data.npy`` (NTU: with the trailing person axis), ``..._gen_z.npy``
and ``..._gen_label.pkl`` (the label vector stacked twice, what Feeder unpacks as (names, labels)) - written to
``<out>/actions``.  Every round of ``--batch_size`` samples per class is one hipGraph replay whose first launch draws
the round's latents, injected noise and truncation latents on the device.  Extra flags: ``--out``, ``--seed`` (every
random input; the reference draws from numpy's unseeded global generator), ``--no-graph`` (the same launches, eagerly).
The files are what ``tools/mmd_actions.py`` reads as ``--data_fake`` / ``--labels_fake``."""
import argparse
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import kinetic_gan_amd  # noqa: E402,F401
from kinetic_gan_amd.generator import Generator  # noqa: E402
from kinetic_gan_amd.sample import Sampler  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--batch_size", type=int, default=10, help="How many samples PER CLASS (each iteration of course)")
    p.add_argument("--latent_dim", type=int, default=512, help="dimensionality of the latent space")
    p.add_argument("--mlp_dim", type=int, default=4, help="mapping network depth")
    p.add_argument("--n_classes", type=int, default=60, help="number of classes for dataset")
    p.add_argument("--label", type=int, default=-1, help="Specific label to generate, -1 for all classes")
    p.add_argument("--t_size", type=int, default=64, help="size of each temporal dimension")
    p.add_argument("--v_size", type=int, default=25, help="size of each spatial dimension (vertices)")
    p.add_argument("--channels", type=int, default=3, help="number of channels (coordinates)")
    p.add_argument("--dataset", type=str, default="ntu", help="dataset")
    p.add_argument("--model", type=str, default="runs/kinetic-gan/models/generator_0.pth", help="path to gen model")
    p.add_argument("--stochastic", action="store_true", help="Generate/Get one sample and verify stochasticity")
    p.add_argument("--stochastic_file", type=str, default="-", help="Read one sample and verify stochasticity")
    p.add_argument("--stochastic_index", type=int, default=0, help="Sample index to get your latent point")
    p.add_argument("--gen_qtd", type=int, default=1000, help="How many samples to generate per class")
    p.add_argument("--trunc", type=float, default=0.95, help="Truncation sigma")
    p.add_argument("--trunc_mode", type=str, default="w", choices=["z", "w", "-"], help="Truncation mode (check paper for details)")
    p.add_argument("--mean_size", type=int, default=1000, help="Samples to estimate mean")
    p.add_argument("--out", type=str, default="runs/kinetic-gan", help="run directory (files go to <out>/actions)")
    p.add_argument("--seed", type=int, default=0, help="seed of every random input")
    p.add_argument("--no-graph", action="store_true", help="run the rounds eagerly instead of replaying a hipGraph")
    return p.parse_args(argv)


def main(argv=None):
    opt = parse_args(argv)
    print(opt)
    if not torch.cuda.is_available():
        raise SystemExit("tools/generate.py needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    actions_out = os.path.join(opt.out, "actions")
    os.makedirs(actions_out, exist_ok=True)
    with open(os.path.join(opt.out, "gen_config.txt"), "w") as f:
        f.write(os.path.basename(__file__) + "|" + str(opt))

    G = Generator(opt.latent_dim, opt.channels, opt.n_classes, opt.t_size, mlp_dim=opt.mlp_dim, dataset=opt.dataset).to(dev)
    G.load_state_dict(torch.load(opt.model, map_location=dev), strict=False)
    if G.graph.num_node[0] != opt.v_size:
        raise SystemExit("--v_size %d does not match the %s skeleton (%d joints)" % (opt.v_size, opt.dataset, G.graph.num_node[0]))

    fixed_z = None
    if opt.stochastic:          # one latent point for every sample
        if opt.stochastic_file != "-":
            fixed_z = torch.as_tensor(np.load(opt.stochastic_file)[opt.stochastic_index], dtype=torch.float32)
        else:
            fixed_z = torch.as_tensor(np.random.RandomState(opt.seed).normal(0, 1, (1, opt.latent_dim)), dtype=torch.float32)
    s = Sampler(G, qtd=opt.batch_size, label=opt.label, seed=opt.seed, trunc=opt.trunc if opt.trunc_mode != "-" else None,
                trunc_mode=opt.trunc_mode, mean_size=opt.mean_size, fixed_z=fixed_z, use_graph=not opt.no_graph)
    imgs, labels, zs = s.generate(opt.gen_qtd)
    imgs, zs = imgs.numpy(), zs.numpy()
    print(len(labels), "samples,", s.step_count, "rounds of", s.n)

    if opt.dataset == "ntu":
        imgs = np.expand_dims(imgs, axis=-1)
    labels = np.concatenate((np.expand_dims(labels, 0), np.expand_dims(labels, 0)), axis=0)
    stem = str(opt.n_classes if opt.label == -1 else opt.label) + "_" + str(opt.gen_qtd) + \
        ("_trunc" + str(opt.trunc) if opt.trunc_mode != "-" else "") + ("_stochastic" if opt.stochastic else "")
    with open(os.path.join(actions_out, stem + "_gen_data.npy"), "wb") as f:
        np.save(f, imgs)
    with open(os.path.join(actions_out, stem + "_gen_z.npy"), "wb") as f:
        np.save(f, zs)
    with open(os.path.join(actions_out, stem + "_gen_label.pkl"), "wb") as f:
        pickle.dump(labels, f)
    print(os.path.join(actions_out, stem + "_gen_data.npy"))
    return actions_out, stem


if __name__ == "__main__":
    main()
