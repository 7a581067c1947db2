"""torch.optim.Adam whose step on the training step's flat gradient buffer is two launches of libarreau_hip.so.

The reference clips with `pl.Trainer(gradient_clip_val=0.5)` (main_diffusion.py:297) and steps torch.optim.Adam over two parameter
groups (lightning_wrappers/diffusion.py:152-218).  PONITA_DIFFUSION.training_step leaves every gradient as a view of ONE buffer;
`ClipAdam.step_flat` hands that buffer to arreau_optimizer_step (arreau_amd/csrc/optim.hip: norm, clip coefficient, non-finite guard
and the Adam update of all 70 tensors), where torch takes a norm, nine scalar launches, a scale, a select and seven multi-tensor
launches.  Everything else is torch.optim.Adam: parameter groups, the LR scheduler's view of them, `state_dict()` /
`load_state_dict()` (the moments are ordinary per-parameter tensors -- views of two flat buffers), and `step()` itself, which stays
the generic path for gradients that are not views of one buffer (and the only one on the CPU).

`EMAOptimizer` keeps an exponential moving average of the weights around any optimizer (the reference's NeMo EMAOptimizer); around a
ClipAdam its update rides in the same launch (arreau_optimizer_step_ema).
"""
import contextlib
import copy
import ctypes
import numbers

import torch


class ClipAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._table = None       # (key, handle)
        self._m_flat = self._v_flat = None

    def __del__(self):
        self._drop_table()

    def _drop_table(self):
        tab = self.__dict__.get("_table")
        if tab is not None:
            try:
                from . import _hip
                _hip.lib().arreau_optimizer_destroy(tab[1])
            except Exception:  # interpreter shutdown
                pass
            self._table = None

    def _flat_entries(self, flat):
        """[(param, offset in `flat`, group index)] when every gradient is a contiguous fp32 view of `flat`; None otherwise."""
        from . import _hip
        if not (flat.is_cuda and flat.dtype == torch.float32 and flat.is_contiguous() and flat.dim() == 1):
            return None
        if len(self.param_groups) > _hip.OPT_MAX_GROUPS:
            return None
        base, base_off = flat.untyped_storage().data_ptr(), flat.storage_offset()
        entries = []
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize") or group.get("capturable") or group.get("differentiable"):
                return None
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not (g.untyped_storage().data_ptr() == base and g.is_contiguous() and g.dtype == torch.float32 and
                        p.dtype == torch.float32 and p.is_contiguous() and p.device == flat.device and not g.is_sparse):
                    return None
                off = g.storage_offset() - base_off
                if off < 0 or off + p.numel() > flat.numel():
                    return None
                entries.append((p, off, gi))
        return entries or None

    def step_flat(self, flat, max_norm=None, mirrors=None, ema=None):
        """Clip `flat` (the buffer all `.grad`s are views of) to `max_norm` and step.  Returns the gradient norm (0-d device tensor),
        or None when the gradients are not laid out that way -- the caller then clips and calls step().
        `mirrors` {parameter: device address}: a second destination for the updated values (HipEngine.train_weight_mirrors).
        `ema` (buffer, decay): a flat fp32 buffer laid out like `flat` whose elements become buffer * decay + (1 - decay) * p in the
        same launch (arreau_optimizer_step_ema; EMAOptimizer.step_flat)."""
        from . import _hip
        entries = self._flat_entries(flat)
        if entries is None:
            return None
        betas = {tuple(g["betas"]) for g in self.param_groups}
        epss = {g["eps"] for g in self.param_groups}
        if len(betas) != 1 or len(epss) != 1:
            return None
        L = _hip.lib()
        mirrors = mirrors or {}
        key = (flat.numel(), tuple((p.data_ptr(), off, gi, mirrors.get(p, 0)) for p, off, gi in entries))
        if self._table is None or self._table[0] != key:
            self._drop_table()
            n = len(entries)
            ptrs = (ctypes.c_void_p * n)(*[p.data_ptr() for p, _, _ in entries])
            mirr = (ctypes.c_void_p * n)(*[mirrors.get(p, None) for p, _, _ in entries])
            numel = (ctypes.c_int64 * n)(*[p.numel() for p, _, _ in entries])
            offs = (ctypes.c_int64 * n)(*[off for _, off, _ in entries])
            grp = (ctypes.c_int32 * n)(*[gi for _, _, gi in entries])
            handle = ctypes.c_void_p()
            _hip.check(L.arreau_optimizer_create(n, ptrs, mirr, numel, offs, grp, len(self.param_groups), flat.numel(), ctypes.byref(handle)),
                       "arreau_optimizer_create")
            self._table = (key, handle)
        if self._m_flat is None or self._m_flat.numel() != flat.numel() or self._m_flat.device != flat.device:
            self._m_flat, self._v_flat = torch.zeros_like(flat), torch.zeros_like(flat)
            # (moments that exist already -- load_state_dict, an earlier step() -- move into the flat buffers below)
        steps = []
        for p, off, _ in entries:
            st = self.state[p]
            m_view = self._m_flat[off:off + p.numel()].view_as(p)
            if "exp_avg" not in st or st["exp_avg"].data_ptr() != m_view.data_ptr():
                v_view = self._v_flat[off:off + p.numel()].view_as(p)
                if "exp_avg" in st:
                    m_view.copy_(st["exp_avg"])
                    v_view.copy_(st["exp_avg_sq"])
                st["exp_avg"], st["exp_avg_sq"] = m_view, v_view
                if "step" not in st:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
            steps.append(st["step"])
        if any(s.is_cuda for s in steps):
            return None   # (a state_dict of torch's fused / capturable Adam: step counts on the device; torch's path handles it)
        first = float(steps[0])
        if any(float(s) != first for s in steps[1:]):
            return None   # (per-parameter step counts that differ: a state_dict stitched together by hand)
        torch._foreach_add_(steps, 1.0)
        args = _hip.AdamArgs()
        args.step = int(first) + 1
        for gi, g in enumerate(self.param_groups):
            lr = g["lr"]
            args.lr[gi] = float(lr)
            args.weight_decay[gi] = float(g["weight_decay"])
        (b1, b2), = betas
        args.beta1, args.beta2, args.eps = float(b1), float(b2), float(next(iter(epss)))
        args.max_norm = float(max_norm) if max_norm else 0.0
        norm = torch.empty((), device=flat.device, dtype=torch.float32)
        if ema is None:
            _hip.check(L.arreau_optimizer_step(self._table[1], _hip.ptr(flat), _hip.ptr(self._m_flat), _hip.ptr(self._v_flat),
                                               ctypes.byref(args), _hip.ptr(norm), _hip.stream_ptr(flat.device)), "arreau_optimizer_step")
        else:
            buf, decay = ema
            assert buf.dtype == torch.float32 and buf.device == flat.device and buf.numel() == flat.numel() and buf.is_contiguous()
            _hip.check(L.arreau_optimizer_step_ema(self._table[1], _hip.ptr(flat), _hip.ptr(self._m_flat), _hip.ptr(self._v_flat),
                                                   ctypes.byref(args), _hip.ptr(buf), float(decay), _hip.ptr(norm),
                                                   _hip.stream_ptr(flat.device)), "arreau_optimizer_step_ema")
        return norm


class EMAOptimizer(torch.optim.Optimizer):
    """An exponential moving average of the weights around any torch.optim.Optimizer: NeMo's EMAOptimizer, which the reference
    carries (lightning_wrappers/callbacks.py:192-392; `EMA(0.99)` is commented out in main_diffusion.py:263-267), with its
    semantics and state_dict format.

    At the first step the average becomes a copy of every parameter of the optimizer's groups (group order, then parameter order),
    taken before the update.  Every step runs the inner step, then -- when `current_step % every_n_steps == 0` --
    ema = decay * ema + (1 - decay) * p, and counts `current_step` up.  A step whose gradient norm was not finite is no exception: the
    average follows the values that step leaves.  `swap_ema_weights()` puts the average into the parameters for the length of a
    block.  The LR scheduler stays on the inner optimizer; anything not defined here is the inner optimizer's.

    The average of a frozen parameter (requires_grad False) is the copy of the first step: the optimizer never changes it.
    Unlike the reference there is no side stream or thread: on the GPU the update runs on the current stream, and on the training
    step's flat gradient buffer it is not a launch of its own at all -- `step_flat` hands the average, homed in a flat buffer laid
    out like the gradients, to ClipAdam's launch (arreau_optimizer_step_ema), where the new parameter value is still in a register.
    Where the flat path declines, arreau_amd.train.optimizer_step calls step(), whose update is the reference's _foreach pair.

    `module`: the PONITA_DIFFUSION the parameters belong to.  Swapping values under its HIP engine would leave the engine on the
    wrong weights, so the swap runs inside `module.parameters_swapped()`."""

    def __init__(self, optimizer, decay, every_n_steps=1, current_step=0, module=None):
        if not isinstance(optimizer, torch.optim.Optimizer):
            raise TypeError(f"EMAOptimizer wraps a torch.optim.Optimizer, not {type(optimizer).__name__}")
        if isinstance(decay, bool) or not isinstance(decay, numbers.Real) or not 0.0 <= decay <= 1.0:
            raise ValueError(f"EMA decay must be a number in [0, 1], got {decay!r}")
        if isinstance(every_n_steps, bool) or not isinstance(every_n_steps, numbers.Integral) or every_n_steps < 1:
            raise ValueError(f"every_n_steps must be an integer >= 1, got {every_n_steps!r}")
        self.optimizer = optimizer
        self.decay = float(decay)
        self.every_n_steps = int(every_n_steps)
        self.current_step = int(current_step)
        self.module = module
        self.ema_params = ()
        self.rebuild_ema_params = True
        self._ema_flat = None

    def __getattr__(self, name):
        if name == "optimizer":  # (not set yet: no recursion through the delegation below)
            raise AttributeError(name)
        return getattr(self.optimizer, name)

    def all_parameters(self):
        return (p for group in self.optimizer.param_groups for p in group["params"])

    def _build_ema(self):
        if self.rebuild_ema_params:
            params = list(self.all_parameters())
            self.ema_params += tuple(p.detach().clone() for p in params[len(self.ema_params):])
            self.rebuild_ema_params = False

    def _should_update_at_step(self):
        return self.current_step % self.every_n_steps == 0

    @torch.no_grad()
    def update(self):
        """ema = decay * ema + (1 - decay) * p (callbacks.py:173-180) for every parameter the optimizer may change.  A frozen one
        (requires_grad False: the module's Fourier projection) never changes, so its average stays the exact copy of the first step
        -- the reference would round it through the recurrence; the fused launch has no slot for it in the flat buffer."""
        pairs = [(e, p.detach()) for p, e in zip(self.all_parameters(), self.ema_params) if p.requires_grad]
        if pairs:
            ema, cur = (list(t) for t in zip(*pairs))
            torch._foreach_mul_(ema, self.decay)
            torch._foreach_add_(ema, cur, alpha=1.0 - self.decay)

    def step(self, closure=None):
        self._build_ema()
        loss = self.optimizer.step(closure)
        if self._should_update_at_step():
            self.update()
        self.current_step += 1
        return loss

    def step_flat(self, flat, max_norm=None, mirrors=None):
        """ClipAdam.step_flat with the average updated in the same launch.  Returns the gradient norm, or None when the flat path
        declines (another optimizer, a gradient that is not a view of `flat`, a trainable parameter with elements but without a
        gradient): the caller then clips and calls step(), which updates the average instead."""
        if not isinstance(self.optimizer, ClipAdam):
            return None
        entries = self.optimizer._flat_entries(flat)
        params = list(self.all_parameters())
        if entries is None or {id(p) for p, _, _ in entries} != {id(p) for p in params if p.requires_grad and p.numel()}:
            return None
        self._build_ema()
        # the average lives in a flat buffer laid out like the gradients, as ClipAdam's moments do; a new gradient buffer (the engine
        # was rebuilt) or a loaded state_dict moves the values into place (frozen parameters keep theirs apart: see update())
        offset = {id(p): off for p, off, _ in entries}
        buf = self._ema_flat
        if (buf is None or buf.numel() != flat.numel() or buf.device != flat.device or
                any(e.data_ptr() != buf[offset[id(p)]:].data_ptr() for p, e in zip(params, self.ema_params) if id(p) in offset)):
            buf = torch.zeros_like(flat)
            homed = []
            for p, e in zip(params, self.ema_params):
                if id(p) in offset:
                    view = buf[offset[id(p)]:offset[id(p)] + p.numel()].view_as(p)
                    view.copy_(e)
                    e = view
                homed.append(e)
            self._ema_flat, self.ema_params = buf, tuple(homed)
        norm = self.optimizer.step_flat(flat, max_norm, mirrors, ema=(buf, self.decay) if self._should_update_at_step() else None)
        if norm is not None:
            self.current_step += 1
        return norm

    def zero_grad(self, set_to_none=True):
        self.optimizer.zero_grad(set_to_none=set_to_none)

    def add_param_group(self, param_group):
        self.optimizer.add_param_group(param_group)
        self.rebuild_ema_params = True

    @staticmethod
    def swap_tensors(tensor1, tensor2):
        tmp = torch.empty_like(tensor1)
        tmp.copy_(tensor1)
        tensor1.copy_(tensor2)
        tensor2.copy_(tmp)

    @torch.no_grad()
    def switch_main_parameter_weights(self):
        for p, e in zip(self.all_parameters(), self.ema_params):
            self.swap_tensors(p.data, e)

    @contextlib.contextmanager
    def swap_ema_weights(self, enabled=True):
        """Within the block the parameters hold the average and the average the training values; both are swapped back on exit,
        on an exception too."""
        if not enabled:
            yield
            return
        guard = self.module.parameters_swapped() if self.module is not None else contextlib.nullcontext()
        with guard:
            self.switch_main_parameter_weights()
            try:
                yield
            finally:
                self.switch_main_parameter_weights()

    def state_dict(self):
        return {"opt": self.optimizer.state_dict(), "ema": self.ema_params, "current_step": self.current_step,
                "decay": self.decay, "every_n_steps": self.every_n_steps}

    def load_state_dict(self, state_dict):
        self.optimizer.load_state_dict(state_dict["opt"])
        params = list(self.all_parameters())
        ema = copy.deepcopy(tuple(state_dict["ema"]))
        self.ema_params = tuple(e.to(p.device) for e, p in zip(ema, params)) + tuple(ema[len(params):])
        self.current_step = state_dict["current_step"]
        self.decay = state_dict["decay"]
        self.every_n_steps = state_dict["every_n_steps"]
        self.rebuild_ema_params = False
