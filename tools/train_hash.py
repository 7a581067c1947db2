"""sha1 of what one training step and one score evaluation of one model compute: the loss, every gradient tensor after one
train_forward / train_backward, conv_stats of that forward, and predict_scores on the same noised batch (for a shape the fused
sampling kernels do not take, arreau_general_network with exact products).  A sibling of tools/determinism.py for A/B runs
of two builds of the library (ARREAU_HIP_LIB selects the other one): equal lines mean equal bits.

    python tools/train_hash.py [--hidden 128 --basis 256 --widening 4 --layers 2 --S 90 --max-neighbors 8 --no-layer-scale] 1 3 7
"""
import argparse
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arreau_amd.checkpoint import make_synthetic_model  # noqa: E402
from arreau_amd.diffusion.diffusion_helpers import crystal_offsets  # noqa: E402
from oracle import geometry as OG  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--hidden", type=int, default=128)
ap.add_argument("--basis", type=int, default=256)
ap.add_argument("--widening", type=int, default=4)
ap.add_argument("--layers", type=int, default=2)
ap.add_argument("--S", type=int, default=90)
ap.add_argument("--max-neighbors", type=int, default=8)
ap.add_argument("--no-layer-scale", action="store_true")
ap.add_argument("num_atoms", type=int, nargs="+", help="atoms of each crystal")
a = ap.parse_args()

sha = lambda v: hashlib.sha1(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]
dev = torch.device("cuda", 0)
extra = {"layer_scale": 0.0} if a.no_layer_scale else {}
m = make_synthetic_model(S=a.S, seed=1234, num_timesteps=100, hidden_dim=a.hidden, basis_dim=a.basis, widening_factor=a.widening,
                         layers=a.layers, max_neighbors=a.max_neighbors, **extra).to(dev)
rng = np.random.RandomState(8)
B, N, S = len(a.num_atoms), sum(a.num_atoms), a.S
lengths = torch.tensor(rng.uniform(3.5, 7.0, size=(B, 3)), dtype=torch.float32)
angles = torch.tensor(np.deg2rad(rng.uniform(75, 105, size=(B, 3))), dtype=torch.float32)
batch = SimpleNamespace(X0=torch.tensor(rng.uniform(0, 1, size=(N, 3)), dtype=torch.float32),
                        A0=torch.tensor(rng.randint(0, S - 1, size=N)), L0=OG.lattice_from_params(lengths, angles).reshape(-1, 3),
                        num_atoms=torch.tensor(a.num_atoms))
timestep = torch.tensor(rng.randint(1, 101, size=B))
g = torch.Generator().manual_seed(4)
noise = (torch.randn(N, 3, generator=g), torch.rand(N, S, generator=g), torch.randn(B, 3, generator=g))

loss, p = m.diffusion_loss(m, batch, m.t_emb, timestep=timestep, noise=noise, return_parts=True, training=True)
eng = m.engine(for_training=True)
stats = eng.conv_stats()
grads = eng.train_backward(p["grad_eps"], p["grad_logits"], p["grad_lengths"])
scores = eng.predict_scores(p["noisy_frac"], p["noisy_types"], p["noisy_lengths"], p["angles"], p["timestep"],
                            crystal_offsets(batch.num_atoms, dev))
st = eng.status(reset=False)  # (synchronises the stream)
print("flags %d edge %s mlp %s conv %d readout %d" % (st["flags"], st["edge_kernel"], st["mlp_kernel"], st["conv_variant"], st["readout_kernel"]))
print("sha1 loss:%s (%.9g)" % (sha(loss), float(loss)))
print("sha1 conv_stats:%s" % sha(stats))
for name in sorted(grads):
    print("sha1 grad %s:%s" % (name, sha(grads[name])))
print("sha1 scores " + " ".join("%s:%s" % (nm, sha(v)) for nm, v in zip(("eps", "logits", "len0"), scores)))
