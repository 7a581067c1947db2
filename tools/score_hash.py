"""sha1 of what the score network computes on a synthetic fused model (S 90, L 2), and which kernels it ran: eps, logits, len0 and
the full status line of one predict_scores, then the state and the status line after a 3-step sample_loop, eager and with
use_graph.  A sibling of tools/train_hash.py for A/B runs of two builds of the library (ARREAU_HIP_LIB selects the other one):
equal lines mean equal bits and equal kernels.  The ARREAU_* switches come from the environment; one process per environment.

    python tools/score_hash.py [--variant EDGE,MLP] [one8] [ragged300] [x26]

Batches: one8 = 1 crystal of 8 atoms; ragged300 = the 13 ragged crystals of tests/test_gpu_conv_proj_forms.py; x26 = 26 crystals
of 20 atoms (520: past the small-launch forms).  All three, on one engine, when none is named.
"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arreau_amd.checkpoint import make_synthetic_model  # noqa: E402
from arreau_amd.diffusion.diffusion_helpers import crystal_offsets  # noqa: E402
from tests.helpers import random_state  # noqa: E402

BATCHES = {"one8": [8], "ragged300": [24, 23, 25, 22, 26, 21, 27, 20, 28, 19, 29, 18, 18], "x26": [20] * 26}
ap = argparse.ArgumentParser()
ap.add_argument("--variant", default="-1,-1", help="set_variant(edge, mlp); -1 keeps")
ap.add_argument("batches", nargs="*", default=list(BATCHES))
a = ap.parse_args()

sha = lambda v: hashlib.sha1(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]
dev = torch.device("cuda", 0)
eng = make_synthetic_model(S=90, seed=1234, layers=2).to(dev).engine()
eng.set_variant(*(int(v) for v in a.variant.split(",")))


def status():
    st = eng.status(reset=False)  # (synchronises the stream)
    return " ".join("%s=%s" % (k, st[k]) for k in sorted(st))


for name in a.batches:
    counts = BATCHES[name]
    B = len(counts)
    d = lambda v: v.to(dev).contiguous()
    frac, types, lengths, angles, na = random_state(90, counts, 41)
    off = crystal_offsets(na, dev)
    scores = eng.predict_scores(d(frac), d(types.to(torch.int32)), d(lengths), d(angles), torch.full((B,), 400, device=dev, dtype=torch.int32), off)
    print("%s scores status %s" % (name, status()))
    print("%s scores sha1 " % name + " ".join("%s:%s" % (nm, sha(v)) for nm, v in zip(("eps", "logits", "len0"), scores)))
    # (drawn like the sampler's start: the loop takes monoclinic angles in degrees)
    frac, types, lengths, angles = (d(x) for x in random_state(90, counts, 43, sampler_like=True)[:4])
    for mode, use_graph in (("eager", False), ("graph", True)):
        state = (frac.clone(), types.to(torch.int32), lengths.clone(), torch.zeros(B, 3, 3, device=dev))
        eng.sample_loop(state[0], state[1], state[2], angles, off, 999, 3, 4242, None, state[3], use_graph=use_graph)
        print("%s loop %s status %s" % (name, mode, status()))
        print("%s loop %s sha1 " % (name, mode) + " ".join("%s:%s" % (nm, sha(v)) for nm, v in zip(("frac", "types", "lengths", "lattice"), state)))
