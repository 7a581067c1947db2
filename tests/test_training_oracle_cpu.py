"""The training oracle (oracle/training.py) runs end to end in float64 -- the reference the GPU shape tests compare the
training step's loss and gradients against -- and agrees with its float32 run to float32 rounding.  CPU only."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import geometry as OG
from oracle import sampler as OS
from oracle import training as TR
from tests.helpers import oracle_from_module, random_state

# float32 rounding carried through a two-layer network and its backward pass: measured 1e-7 (loss) and 1e-6 (largest
# gradient error relative to that tensor's largest entry) at this shape
LOSS_REL = 1e-6
REL = 1e-5


def _model():
    from arreau_amd.checkpoint import make_synthetic_model
    return make_synthetic_model(S=12, seed=5, num_timesteps=20, hidden_dim=16, basis_dim=16, widening_factor=2, layers=2)


def test_float64_training_loss_and_gradients_match_float32():
    m = _model()
    S, T = 12, 20
    rng = np.random.RandomState(3)
    num_atoms = torch.tensor([3, 5, 1])
    B, N = len(num_atoms), int(num_atoms.sum())
    lengths = torch.tensor(rng.uniform(3.5, 7.0, size=(B, 3)))
    angles = torch.tensor(np.deg2rad(rng.uniform(75, 105, size=(B, 3))))
    lattice0 = OG.lattice_from_params(lengths, angles)
    frac0 = torch.tensor(rng.uniform(0, 1, size=(N, 3)))
    types0 = torch.tensor(rng.randint(0, S - 1, size=N))
    timestep = torch.tensor([1, 10, T])
    g = torch.Generator().manual_seed(4)
    noise = (torch.randn(N, 3, generator=g, dtype=torch.float64), torch.rand(N, S, generator=g, dtype=torch.float64),
             torch.randn(B, 3, generator=g, dtype=torch.float64))
    res = {}
    for dtype in (torch.float32, torch.float64):
        om = oracle_from_module(m, dtype)
        for v in om.sd.values():
            if v.is_floating_point() and v.numel() > 0:
                v.requires_grad_(True)
        c = lambda x: x.to(dtype)
        loss = TR.diffusion_loss(om, c(frac0), types0, c(lattice0), num_atoms, timestep, *(c(z) for z in noise))
        assert loss.dtype == dtype
        loss.backward()
        res[dtype] = (float(loss.detach()), {k: v.grad for k, v in om.sd.items() if v.requires_grad and v.grad is not None})
    (l32, g32), (l64, g64) = res[torch.float32], res[torch.float64]
    assert abs(l32 - l64) <= LOSS_REL * max(1.0, abs(l64)), (l32, l64)
    assert sorted(g32) == sorted(g64) and len(g64) >= 9 + 10 * 2
    for name, w in g64.items():
        assert w.dtype == torch.float64
        err = float((g32[name].double() - w).abs().max())
        assert err <= REL * max(float(w.abs().max()), 1e-7), (name, err, float(w.abs().max()))


def test_float64_predict_scores_matches_float32():
    m = _model()
    state = random_state(12, [6, 1, 4], 2)
    frac, types, lengths, angles, na = state
    B, N = len(na), frac.shape[0]
    batch = torch.arange(B).repeat_interleave(na)
    out = {}
    for dtype in (torch.float32, torch.float64):
        om = oracle_from_module(m, dtype)
        c = lambda x: x.to(dtype)
        out[dtype] = OS.predict_scores(om, c(frac), F.one_hot(types, 12), torch.full((N,), 7), na, c(lengths), c(angles),
                                       batch)
    for name, a, b in zip(("eps", "logits", "len0"), out[torch.float32], out[torch.float64]):
        assert a.dtype == torch.float32 and b.dtype == torch.float64, name
        err = float((a.double() - b).abs().max())
        assert err <= REL * max(1.0, float(b.abs().max())), (name, err)
