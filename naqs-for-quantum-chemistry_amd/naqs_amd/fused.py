"""Fused HIP evaluation of log psi for a batch of keys (``naqs_net_*`` entry points).

The product path of the metric's "log-psi eval": two kernels instead of ~200 eager launches.
Supported architecture families:
  * what the reference's published runs use (batch_train.sh:14): one hidden layer per amplitude block (a multiple of 16,
    <= 128 units), a single phase block (``aggregate_phase=False``) of 1..8 hidden layers <= 512 wide; with this single phase
    block the amplitude blocks may also have 2..4 hidden layers of one width (``-n_layer``; ``naqs_net_create_amp_layers``);
  * the reference's default ansatz (experiments/run.py:11-31): the same amplitude blocks and one phase block per orbital
    pair (``aggregate_phase=True``), each with one hidden layer (multiple of 16, <= 128 units); or every amplitude and phase
    block with the same 2..4 hidden layers (``-n_layer``), one width per kind of block (``naqs_net_create_agg_layers``);
both with or without the phase spin symmetry (``-phase_sym``, nade.py:281, 507-533, 590-610: spin-ordered inputs of the phase
block(s), 3 outputs, the sign shift — since round 5);
  * combined amplitude-phase blocks with a single phase (``-single_phase -comb_amp_phase``, nade.py:294-303, 555-560): no phase
    MLP, the last one-hidden-layer amplitude block's output layer also carries the phase rows (``naqs_net_create_combined``);
<= 16 orbital pairs.  Anything else (combined blocks with ``aggregate_phase=True`` or deeper blocks, amplitude and phase blocks of
different depths with ``aggregate_phase=True``, look-up-table blocks) raises
``NotImplementedError`` — callers then stay on the PyTorch modules (same numbers, more launches), and ``wavefunction.fused()``
says so on stdout.
"""
import ctypes
import os

import torch

from . import _lib
from .hamiltonian import _stream_ptr


class _LogAmp(torch.autograd.Function):
    """log|psi|(keys) with the amplitude blocks' forward and backward as HIP kernels
    (``naqs_net_logamp`` / ``naqs_net_amp_backward``)."""

    @staticmethod
    def forward(ctx, fused, keys, *amp_params):
        M = keys.shape[0]
        out = torch.empty(M, dtype=torch.float32, device=keys.device)
        st = fused._lib.naqs_net_logamp(fused._h, M, keys.data_ptr(), out.data_ptr(), _stream_ptr(fused.device))
        _lib.check(st, "naqs_net_logamp")
        ctx.fused, ctx.keys = fused, keys
        ctx.shapes = [p.shape for p in amp_params]
        return out

    @staticmethod
    def backward(ctx, g):
        fused, keys = ctx.fused, ctx.keys
        g = g.to(torch.float32).contiguous()
        flat = torch.empty(fused.n_amp_params, dtype=torch.float32, device=keys.device)
        st = fused._lib.naqs_net_amp_backward(fused._h, keys.shape[0], keys.data_ptr(), g.data_ptr(), flat.data_ptr(),
                                              _stream_ptr(fused.device))
        _lib.check(st, "naqs_net_amp_backward")
        grads, off = [], 0
        for shp in ctx.shapes:
            n = shp.numel()
            grads.append(flat[off:off + n].view(shp))
            off += n
        return (None, None, *grads)


def _accumulate(p, grad):
    if p.grad is None:
        p.grad = grad
    else:
        p.grad.add_(grad)


def _seed64(seed):
    """A Python seed as the uint64 the library takes."""
    return int(seed) & (2 ** 64 - 1)


class FusedLogPsi:
    def __init__(self, wavefunction):
        wf, m = wavefunction, wavefunction.model
        if m.device.type != "cuda":
            raise _lib.NaqsError("FusedLogPsi needs the network on a HIP device (no CPU fallback)")
        self.aggregate = bool(m.aggregate_phase)
        self.phase_sym = bool(getattr(m, "use_phase_spin_sym", False))
        # -comb_amp_phase: the single-phase form with one hidden layer per block runs on the kernels (naqs_net_create_combined)
        self.comb = bool(getattr(m, "combined_amp_phase_blocks", False))
        amp_lin = m.amp_layers[0].linears()
        # 1 hidden layer; or 2..4 of one width with a single phase block (naqs_net_create_amp_layers), or with per-pair phase
        # blocks of the same depth (naqs_net_create_agg_layers)
        self.amp_depth = len(amp_lin) - 1
        if self.comb and (self.aggregate or self.amp_depth != 1):
            raise NotImplementedError("fused log-psi: combined amplitude-phase blocks with aggregate_phase=True or more than one "
                                      "hidden layer (no published script uses them) run as PyTorch modules")
        if len(m.phase_layers) != (0 if self.comb else (m.P if self.aggregate else 1)):
            raise NotImplementedError("fused log-psi: unexpected number of phase blocks")
        ph_depth = len(m.phase_layers[0].linears()) - 1 if self.aggregate else 0
        deep_ok = (2 <= self.amp_depth <= _lib.NET_MAX_AMP_LAYERS and len({lin.out_features for lin in amp_lin[:-1]}) == 1
                   and (not self.aggregate or ph_depth == self.amp_depth))
        if self.amp_depth != 1 and not deep_ok:
            raise NotImplementedError("fused log-psi: amplitude blocks need exactly one hidden layer")
        ha = m.amp_layers[0].linears()[0].out_features
        if ha % 16 or ha > 128:
            raise NotImplementedError(f"fused log-psi: amplitude hidden width {ha} (a multiple of 16, <= 128, is supported)")
        if m.P > _lib.NET_MAX_PAIRS or m.P < 2:
            raise NotImplementedError("fused log-psi: 2..16 orbital pairs")
        hidden = [] if self.comb else [lin.out_features for lin in m.phase_layers[0].linears()[:-1]]
        if self.comb:
            pass
        elif self.aggregate:
            if len(hidden) != self.amp_depth or len(set(hidden)) != 1 or hidden[0] % 16 or hidden[0] > 128:
                raise NotImplementedError("fused log-psi: aggregate_phase=True with other than one phase hidden layer per "
                                          f"block of a multiple of 16, <= 128 units (got {hidden}); deeper phase blocks need the "
                                          "amplitude blocks' depth and one width")
        elif not 1 <= len(hidden) <= _lib.NET_MAX_PHASE_LAYERS or max(hidden) > 512:
            raise NotImplementedError("fused log-psi: 1..8 phase hidden layers of width <= 512")
        self._lib = _lib.load_library()
        self.wf = wf
        self.device = m.device
        cfg = _lib.NetConfig()
        cfg.n_qubits = m.N
        cfg.n_alpha = m.n_alpha_up if m.use_restricted_hilbert else -1
        cfg.n_beta = m.n_beta_up if m.use_restricted_hilbert else -1
        cfg.masking = m.masking.value
        cfg.use_amp_spin_sym = int(m.use_amp_spin_sym)
        cfg.amp_hidden = m.amp_layers[0].linears()[0].out_features
        cfg.n_phase_hidden = len(hidden)
        for i, h in enumerate(hidden):
            cfg.phase_hidden[i] = h
        for i, q in enumerate(wf.qubit2model_permutation):
            cfg.qubit2model[i] = int(q)
        cfg.aggregate_phase = int(self.aggregate)
        cfg.use_phase_spin_sym = int(self.phase_sym)          # -phase_sym with one phase block (nade.py:281, 507-533, 590-610)
        self._h = ctypes.c_void_p(None)
        if self.comb:
            st = self._lib.naqs_net_create_combined(ctypes.byref(cfg), self.device.index or 0, ctypes.byref(self._h))
            _lib.check(st, "naqs_net_create_combined")
        elif self.amp_depth == 1:
            st = self._lib.naqs_net_create(ctypes.byref(cfg), self.device.index or 0, ctypes.byref(self._h))
            _lib.check(st, "naqs_net_create")
        elif self.aggregate:
            st = self._lib.naqs_net_create_agg_layers(ctypes.byref(cfg), self.amp_depth, self.device.index or 0, ctypes.byref(self._h))
            _lib.check(st, "naqs_net_create_agg_layers")
        else:
            st = self._lib.naqs_net_create_amp_layers(ctypes.byref(cfg), self.amp_depth, self.device.index or 0, ctypes.byref(self._h))
            _lib.check(st, "naqs_net_create_amp_layers")
        n = ctypes.c_int64(0)
        _lib.check(self._lib.naqs_net_param_count(self._h, ctypes.byref(n)), "naqs_net_param_count")
        self.n_params = n.value
        self._samp = None
        self._grad_flat, self._grad_views = None, None
        self.train_mode = os.environ.get("NAQS_TRAIN_MODE", "hip")     # "hip" | "blas" (phase MLP through torch/rocBLAS)
        if self.aggregate or self.phase_sym or self.comb:
            self.train_mode = "hip"                                     # (the per-pair phase blocks / spin-ordered inputs / phase rows have no BLAS formulation here)
        assert self.n_params == sum(p.numel() for p in m.parameters()), "parameter layout mismatch"
        _lib.check(self._lib.naqs_net_amp_param_count(self._h, ctypes.byref(n)), "naqs_net_amp_param_count")
        self.n_amp_params = n.value
        self._amp_params = [p for blk in m.amp_layers for p in blk.parameters()]
        assert self.n_amp_params == sum(p.numel() for p in self._amp_params), "amplitude parameter layout mismatch"
        if not self.comb:
            # key bits feeding the phase block (alpha then beta occupations of model pairs 0..P-2) and the last pair's outcome
            q2m = [int(q) for q in wf.qubit2model_permutation]
            P = m.P
            self._phase_shifts = torch.tensor([q2m[2 * k] for k in range(P - 1)] + [q2m[2 * k + 1] for k in range(P - 1)],
                                              dtype=torch.int64, device=self.device)
            self._last_a, self._last_b = q2m[2 * (P - 1)], q2m[2 * (P - 1) + 1]
        self.refresh()

    def refresh(self, amp_only=False):
        """Re-pack the current network parameters (after every optimiser step).  ``amp_only`` packs just the
        amplitude blocks — all that sampling and the training forward/backward need; the phase layers are then
        stale for ``log_psi`` / ``log_psi_and_local_energy`` until a full refresh."""
        all_params = self.wf.param_list()
        flat = getattr(self.wf, "_flat_params", None)
        if flat is None or not self.wf._views_of(flat, all_params):       # parameters not (or no longer) flattened: gather
            params = self._amp_params if amp_only else all_params
            flat = torch.cat([p.detach().reshape(-1) for p in params]).to(torch.float32).contiguous()
        fn = self._lib.naqs_net_set_amp_weights if amp_only else self._lib.naqs_net_set_weights
        _lib.check(fn(self._h, flat.data_ptr(), flat.numel(), _stream_ptr(self.device)), "naqs_net_set_weights")
        self._flat = flat          # keep alive until the async copy has been consumed

    # ---- what the training calls share: the flat gradient, the one-call step's outputs, FlatAdam's arguments ----
    def _ensure_grad_flat(self):
        """The persistent flat gradient buffer the backward kernels write (float32 [n_params], state_dict order) and its
        per-parameter views, both made once.  -> the buffer"""
        if self._grad_flat is None:
            self._grad_flat = torch.empty(self.n_params, dtype=torch.float32, device=self.device)
            self._grad_views, off = [], 0
            for p in self.wf.param_list():
                n = p.numel()
                self._grad_views.append(self._grad_flat[off:off + n].view(p.shape))
                off += n
        return self._grad_flat

    def _table_buffers(self, cap):
        """The cap-sized outputs of ``vmc_step`` / ``vmc_run`` live in per-handle buffers (allocated once per cap: eight
        allocator calls per step were ~15 us of host time on a 0.2 ms step); they are valid until the next step of this
        handle.  -> (counts, probs, weights, log psi, E_loc, g)"""
        ob = getattr(self, "_onecall_bufs", None)
        if ob is None or ob[0] != cap:
            dev = self.device
            ob = self._onecall_bufs = (cap, torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.float32, device=dev),
                                       torch.empty(cap, dtype=torch.float64, device=dev), torch.empty((cap, 2), dtype=torch.float32, device=dev),
                                       torch.empty((cap, 2), dtype=torch.float64, device=dev), torch.empty((cap, 2), dtype=torch.float32, device=dev))
        return ob[1:]

    def _adam_args(self, adam, who):
        """A ``FlatAdam`` on this network's flat vector as the library takes it: -> ((parameters, exp_avg, exp_avg_sq) pointers,
        (lr, beta1, beta2, eps, weight_decay), the number of its next step)."""
        if adam._flat.numel() != self.n_params:
            raise ValueError(f"{who}: the optimiser's flat vector is not this network's")
        grp = next(g_ for g_ in adam.param_groups if g_['params'])
        hyper = (float(grp['lr']), float(grp['betas'][0]), float(grp['betas'][1]), float(grp['eps']), float(grp['weight_decay']))
        return (adam._flat.data_ptr(), adam._m.data_ptr(), adam._v.data_ptr()), hyper, adam._t + 1

    def _adam_stepped(self, adam, t):
        """The library applied step ``t`` of ``adam`` and re-packed the weights from its flat vector."""
        if not adam.state:
            adam._bind_state()
        adam._t = t
        adam._opt_called = True          # (what torch's LR schedulers look at to see that a step preceded theirs)
        self._flat = adam._flat

    def log_psi_train(self, keys):
        """Differentiable log psi [M, 2] of int64 device keys: amplitude blocks through the HIP forward/backward
        pair, the phase MLP (three Linear layers) through PyTorch/rocBLAS.  Same function of the parameters as
        ``wavefunction.log_psi(states)``."""
        m = self.wf.model
        if self.aggregate or self.phase_sym or self.comb:
            raise NotImplementedError("log_psi_train (autograd.Function form) for aggregate_phase / phase-symmetric / combined-block "
                                      "networks: use forward_saved / backward_saved")
        keys = keys.contiguous()
        log_amp = _LogAmp.apply(self, keys, *self._amp_params)
        x = ((keys.unsqueeze(-1) >> self._phase_shifts) & 1).to(torch.float32).mul_(2.0).sub_(1.0)
        out = m.phase_layers[0](x)                                                   # nade.py:563-569
        occ = ((keys >> self._last_a) & 1) + 2 * ((keys >> self._last_b) & 1)
        phase = out.gather(1, occ.unsqueeze(1)).squeeze(1)
        return torch.stack([log_amp, phase], -1)

    # ---- training step without the autograd engine --------------------------------------------------------
    @torch.no_grad()
    def forward_saved(self, keys, out=None):
        """log psi [M, 2] of int64 device keys, evaluated without recording an autograd graph, plus the token
        ``backward_saved`` needs.  ``mode="hip"`` (default): ``naqs_net_train_forward`` — the inference kernels, the
        phase activations stay in the handle (``out``: a contiguous float32 [M, 2] to write to).  ``mode="blas"``: HIP
        amplitude kernels + one addmm/relu per phase layer."""
        keys = keys.contiguous()
        M = keys.shape[0]
        if self.train_mode == "hip":
            log_psi = torch.empty((M, 2), dtype=torch.float32, device=self.device) if out is None else out
            st = self._lib.naqs_net_train_forward(self._h, M, keys.data_ptr(), log_psi.data_ptr(), _stream_ptr(self.device))
            _lib.check(st, "naqs_net_train_forward")
            return log_psi, (keys, None, None)
        m = self.wf.model
        log_amp = torch.empty(M, dtype=torch.float32, device=self.device)
        st = self._lib.naqs_net_logamp(self._h, M, keys.data_ptr(), log_amp.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_net_logamp")
        lin = m.phase_layers[0].linears()
        x = torch.empty((M, lin[0].in_features), dtype=torch.float32, device=self.device)
        occ = torch.empty((M, 1), dtype=torch.int64, device=self.device)
        st = self._lib.naqs_net_phase_inputs(self._h, M, keys.data_ptr(), x.data_ptr(), occ.data_ptr(),
                                             _stream_ptr(self.device))
        _lib.check(st, "naqs_net_phase_inputs")
        acts = [x]
        for layer in lin[:-1]:
            acts.append(torch.addmm(layer.bias, acts[-1], layer.weight.t()).relu_())
        out = torch.addmm(lin[-1].bias, acts[-1], lin[-1].weight.t())
        log_psi = torch.stack([log_amp, out.gather(1, occ).squeeze(1)], -1)
        return log_psi, (keys, acts, occ)

    @torch.no_grad()
    def forward_saved_with_local_energy(self, ham, keys, weights):
        """``forward_saved`` (HIP mode) and the local energies of the same table in one library call
        (``naqs_net_train_forward_eloc``): -> (log psi [M, 2] f32, saved token, E_loc [M, 2] f64, sums [4] f64)."""
        keys = keys.contiguous()
        M = keys.shape[0]
        log_psi = torch.empty((M, 2), dtype=torch.float32, device=self.device)
        eloc = torch.empty((M, 2), dtype=torch.float64, device=self.device)
        sums = torch.empty(4, dtype=torch.float64, device=self.device)
        w = weights.to(device=self.device, dtype=torch.float64).contiguous()
        st = self._lib.naqs_net_train_forward_eloc(self._h, ham._h, M, keys.data_ptr(), w.data_ptr(), log_psi.data_ptr(),
                                                   eloc.data_ptr(), sums.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_net_train_forward_eloc")
        return log_psi, (keys, None, None), eloc, sums

    def vmc_loss_grad(self, e_loc, weights, sums, with_energy=False):
        """g [M, 2] float32 = d loss / d (log|psi|, phase) of the VMC loss (``naqs_vmc_loss_grad``); with
        ``with_energy`` also the device pair (<E>, Var) of energy.py:372-375 from the same launch
        (``naqs_vmc_loss_grad_ev``) -> (g, ev float64 [2])."""
        M = e_loc.shape[0]
        g = torch.empty((M, 2), dtype=torch.float32, device=self.device)
        if with_energy:
            ev = torch.empty(2, dtype=torch.float64, device=self.device)
            st = self._lib.naqs_vmc_loss_grad_ev(M, e_loc.data_ptr(), weights.data_ptr(), sums.data_ptr(), g.data_ptr(),
                                                 ev.data_ptr(), _stream_ptr(self.device))
            _lib.check(st, "naqs_vmc_loss_grad_ev")
            return g, ev
        st = self._lib.naqs_vmc_loss_grad(M, e_loc.data_ptr(), weights.data_ptr(), sums.data_ptr(), g.data_ptr(),
                                          _stream_ptr(self.device))
        _lib.check(st, "naqs_vmc_loss_grad")
        return g

    @torch.no_grad()
    def backward_from_local_energy(self, saved, e_loc, weights, sums):
        """``vmc_loss_grad(..., with_energy=True)`` + ``backward_saved`` as ONE library call
        (``naqs_net_train_backward_vmc``): the loss gradient, its amplitude column and the output layer's delta come out of
        one launch instead of three.  -> (g [M, 2] f32, ev f64 [2]); the parameters' ``.grad`` are set like
        ``backward_saved`` does.  Needs the token of ``forward_saved*`` in HIP mode and parameters without gradients."""
        keys = saved[0]
        M = keys.shape[0]
        params = self.wf.param_list()
        if saved[1] is not None or not all(p.grad is None for p in params):
            g, ev = self.vmc_loss_grad(e_loc, weights, sums, with_energy=True)
            self.backward_saved(saved, g)
            return g, ev
        flat = self._ensure_grad_flat()
        g = torch.empty((M, 2), dtype=torch.float32, device=self.device)
        ev = torch.empty(2, dtype=torch.float64, device=self.device)
        st = self._lib.naqs_net_train_backward_vmc(self._h, M, keys.data_ptr(), e_loc.data_ptr(), weights.data_ptr(), sums.data_ptr(),
                                                   g.data_ptr(), ev.data_ptr(), flat.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_net_train_backward_vmc")
        for p, gv in zip(params, self._grad_views):
            p.grad = gv
        return g, ev

    @torch.no_grad()
    def backward_saved(self, saved, g):
        """Accumulate d/d theta sum_i (g[i, 0] log|psi_i| + g[i, 1] phase_i) into the ``.grad`` of every network
        parameter: ``naqs_net_amp_backward`` for the amplitude blocks, the phase MLP's chain rule as plain GEMMs
        (what autograd would run for three Linear layers, without building or walking a graph)."""
        keys, acts, occ = saved
        m = self.wf.model
        g = g.to(torch.float32)
        if acts is None:                     # naqs_net_train_backward: every gradient in one flat buffer
            g = g.contiguous()
            params = self.wf.param_list()
            fresh = all(p.grad is None for p in params)
            # the usual case (zero_grad before every step): the kernels write straight into the persistent flat buffer
            flat = (self._ensure_grad_flat() if fresh
                    else torch.empty(self.n_params, dtype=torch.float32, device=self.device))
            st = self._lib.naqs_net_train_backward(self._h, keys.shape[0], keys.data_ptr(), g.data_ptr(), flat.data_ptr(),
                                                   _stream_ptr(self.device))
            _lib.check(st, "naqs_net_train_backward")
            if fresh:
                for p, gv in zip(params, self._grad_views):
                    p.grad = gv
            else:
                off = 0
                for p in params:
                    n = p.numel()
                    _accumulate(p, flat[off:off + n].view(p.shape))
                    off += n
            return
        flat = torch.empty(self.n_amp_params, dtype=torch.float32, device=self.device)
        ga = g[:, 0].contiguous()
        st = self._lib.naqs_net_amp_backward(self._h, keys.shape[0], keys.data_ptr(), ga.data_ptr(), flat.data_ptr(),
                                              _stream_ptr(self.device))
        _lib.check(st, "naqs_net_amp_backward")
        off = 0
        for p in self._amp_params:
            n = p.numel()
            _accumulate(p, flat[off:off + n].view(p.shape))
            off += n
        lin = m.phase_layers[0].linears()
        delta = torch.zeros((keys.shape[0], lin[-1].out_features), dtype=torch.float32, device=self.device)
        delta.scatter_(1, occ, g[:, 1:2])
        for l in range(len(lin) - 1, -1, -1):
            _accumulate(lin[l].weight, delta.t() @ acts[l])
            _accumulate(lin[l].bias, delta.sum(0))
            if l > 0:
                delta = (delta @ lin[l].weight).mul_(acts[l] > 0)

    # ---- natural gradient in sample space (minSR): naqs_net_sr_gram / naqs_net_sr_direction ----------------
    def _sr_check(self):
        if self.comb or self.amp_depth != 1:
            raise NotImplementedError("natural gradient (minSR): single-phase and aggregate-phase networks with one hidden layer per "
                                      "block only (combined blocks share W1 between amplitude and phase; deeper blocks are not built)")

    @torch.no_grad()
    def sr_gram(self, saved, weights, g, diag_shift, uncentred=False):
        """The two M x M systems of the natural-gradient step for the table of ``forward_saved`` (HIP mode; ``saved`` its token):
        -> (T_a + lambda I, T_phi + lambda I, y_a, y_phi), float64 on the device, T = D (G - m 1^T - 1 m^T + c) D with G the Gram
        matrix of the per-sample gradients of log|psi| (phase), D = diag(sqrt w), m = G w, c = w^T G w, lambda = ``diag_shift``
        x the mean diagonal of T, y = g[:, k] / (2 sqrt w).  ``uncentred``: -> (G_a, G_phi) alone (tests, measurements).
        Memory: 16 M^2 bytes for the two matrices; M <= 32768."""
        self._sr_check()
        keys = saved[0]
        if saved[1] is not None:
            raise NotImplementedError("sr_gram needs the token of forward_saved in HIP mode")
        M = keys.shape[0]
        Ta = torch.empty((M, M), dtype=torch.float64, device=self.device)
        Tp = torch.empty((M, M), dtype=torch.float64, device=self.device)
        if uncentred:
            st = self._lib.naqs_net_sr_gram_uncentred(self._h, M, keys.data_ptr(), Ta.data_ptr(), Tp.data_ptr(), _stream_ptr(self.device))
            _lib.check(st, "naqs_net_sr_gram_uncentred")
            return Ta, Tp
        w = weights.to(device=self.device, dtype=torch.float64).contiguous()
        g = g.to(device=self.device, dtype=torch.float32).contiguous()
        ya = torch.empty(M, dtype=torch.float64, device=self.device)
        yp = torch.empty(M, dtype=torch.float64, device=self.device)
        st = self._lib.naqs_net_sr_gram(self._h, M, keys.data_ptr(), w.data_ptr(), g.data_ptr(), float(diag_shift), Ta.data_ptr(),
                                        Tp.data_ptr(), ya.data_ptr(), yp.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_net_sr_gram")
        return Ta, Tp, ya, yp

    @torch.no_grad()
    def sr_direction(self, saved, weights, xa, xphi, out=None):
        """d theta = X_a^T x_a + X_phi^T x_phi as a flat float32 vector in state_dict order (``naqs_net_sr_direction``): the
        seeds s_i = sqrt(w_i) x_i - w_i sum_j sqrt(w_j) x_j per column, then the training backward with them."""
        self._sr_check()
        keys = saved[0]
        M = keys.shape[0]
        w = weights.to(device=self.device, dtype=torch.float64).contiguous()
        xa = xa.to(device=self.device, dtype=torch.float64).contiguous()
        xphi = xphi.to(device=self.device, dtype=torch.float64).contiguous()
        if out is None:
            out = torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        st = self._lib.naqs_net_sr_direction(self._h, M, keys.data_ptr(), w.data_ptr(), xa.data_ptr(), xphi.data_ptr(), out.data_ptr(),
                                             _stream_ptr(self.device))
        _lib.check(st, "naqs_net_sr_direction")
        return out

    @torch.no_grad()
    def sr_jvp(self, saved, v):
        """(A v, B v) for the table of ``forward_saved`` (HIP mode; ``saved`` its token) and a flat vector ``v`` [n_params] in
        state_dict order (``naqs_net_sr_jvp``): float64 [M] on the device, uncentred.  A = d log|psi| / d theta, B = d phase / d theta;
        no Jacobian is formed (per layer the factors of ``sr_gram`` against v's slice)."""
        self._sr_check()
        keys = saved[0]
        if saved[1] is not None:
            raise NotImplementedError("sr_jvp needs the token of forward_saved in HIP mode")
        M = keys.shape[0]
        v = v.to(device=self.device, dtype=torch.float32).contiguous()
        if v.shape != (self.n_params,):
            raise ValueError(f"sr_jvp: v has shape {tuple(v.shape)}, not ({self.n_params},)")
        ua = torch.empty(M, dtype=torch.float64, device=self.device)
        up = torch.empty(M, dtype=torch.float64, device=self.device)
        st = self._lib.naqs_net_sr_jvp(self._h, M, keys.data_ptr(), v.data_ptr(), ua.data_ptr(), up.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_net_sr_jvp")
        return ua, up

    @torch.no_grad()
    def sr_solve(self, Ta, Tp, ya, yp):
        """T x = y for the systems of ``sr_gram`` by the library's blocked float64 Cholesky (``naqs_net_sr_solve``) -> (x_a, x_phi,
        info).  ``Ta`` and ``Tp`` are OVERWRITTEN: on return their lower triangles (with the diagonal) hold the factors L, the
        strict upper triangles are unspecified.  ``info``: int32 device tensor [2], LAPACK's potrf convention per system (0, or
        p + 1 for the first pivot p that is not positive); a failed system's x is NaN throughout.  ``Tp = yp = None``: one system,
        x_phi is None.  Any network family; no training forward is needed.  One solve at a time per network (handle scratch)."""
        two = Tp is not None
        if two != (yp is not None):
            raise ValueError("sr_solve: Tp and yp come together or not at all")
        M = Ta.shape[0]
        for T, y in ((Ta, ya), (Tp, yp))[:2 if two else 1]:
            if T.dtype != torch.float64 or y.dtype != torch.float64 or not T.is_contiguous() or not y.is_contiguous() \
                    or T.shape != (M, M) or y.shape != (M,) or T.device != self.device or y.device != self.device:
                raise ValueError("sr_solve: contiguous float64 [M, M] matrices and [M] right-hand sides on the network's device")
        xa = torch.empty(M, dtype=torch.float64, device=self.device)
        xp = torch.empty(M, dtype=torch.float64, device=self.device) if two else None
        info = torch.empty(2, dtype=torch.int32, device=self.device)
        st = self._lib.naqs_net_sr_solve(self._h, M, Ta.data_ptr(), Tp.data_ptr() if two else None, ya.data_ptr(),
                                         yp.data_ptr() if two else None, xa.data_ptr(), xp.data_ptr() if two else None,
                                         info.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_net_sr_solve")
        return xa, xp, info

    def log_psi(self, keys, out=None):
        """keys: int64 device tensor [M] (uint64 bit patterns, qubit order) -> float32 [M, 2]."""
        M = keys.shape[0]
        if out is None:
            out = torch.empty((M, 2), dtype=torch.float32, device=self.device)
        st = self._lib.naqs_net_logpsi(self._h, M, keys.contiguous().data_ptr(), out.data_ptr(),
                                       _stream_ptr(self.device))
        _lib.check(st, "naqs_net_logpsi")
        return out

    def exact_local_energy(self, ham, keys_buf, logpsi_buf, M, row_begin, n_rows, capacity, weights=None, out=None, sums_out=None):
        """Exact local energies of table rows [row_begin, row_begin + n_rows) with psi of the connected states the table
        lacks from THIS network's inference forward, in one library call (``naqs_exact_eloc``;
        ``DevicePauliHamiltonian.exact_local_energy``).  ``logpsi_buf[:M]`` holds log psi of the table from a forward of the
        current parameters (``forward_saved(keys, out=logpsi_buf[:M])``).
        -> (E_loc float64 [n_rows, 2], sums float64 [4] or None, count, overflow)."""
        return ham.exact_local_energy(self._h, keys_buf, logpsi_buf, M, row_begin, n_rows, capacity, weights=weights, out=out,
                                      sums_out=sums_out)

    def log_psi_and_local_energy(self, ham, keys, weights=None, log_psi_out=None, eloc_out=None, sums_out=None):
        """keys -> (log psi float32 [M, 2], E_loc float64 [M, 2][, sums float64 [4]]) in one library call
        (``naqs_logpsi_eloc``): the E_loc stage is fed by the log-psi kernels, no preparation kernel."""
        M = keys.shape[0]
        if log_psi_out is None:
            log_psi_out = torch.empty((M, 2), dtype=torch.float32, device=self.device)
        if eloc_out is None:
            eloc_out = torch.empty((M, 2), dtype=torch.float64, device=self.device)
        w_ptr = s_ptr = None
        if weights is not None:
            weights = weights.to(device=self.device, dtype=torch.float64).contiguous()
            if sums_out is None:
                sums_out = torch.empty(4, dtype=torch.float64, device=self.device)
            w_ptr, s_ptr = weights.data_ptr(), sums_out.data_ptr()
        st = self._lib.naqs_logpsi_eloc(self._h, ham._h, M, keys.contiguous().data_ptr(), w_ptr,
                                        log_psi_out.data_ptr(), eloc_out.data_ptr(), s_ptr, _stream_ptr(self.device))
        _lib.check(st, "naqs_logpsi_eloc")
        return (log_psi_out, eloc_out, sums_out) if weights is not None else (log_psi_out, eloc_out)

    def sample(self, n_samples, seed, max_unique, with_weights=False):
        """Draw ``n_samples`` from |psi|^2 on the device (``naqs_net_sample``): -> (keys int64 [M] in qubit order,
        counts int64 [M], probs float32 [M]), M unique bit-strings in (prefix, outcome) order; ``with_weights`` appends
        the float64 weights counts / sum(counts) written by the sampler's last launch (``naqs_net_sample_weighted``).
        Raises ``MaxBatchSizeExceededError`` when more than ``max_unique`` prefixes are alive at some level
        (nade.py:710-712).  One host synchronisation (to learn M); the results are views of buffers allocated for
        this call (copies only when they would pin a much larger buffer)."""
        from .nade import MaxBatchSizeExceededError
        cap = int(max_unique)
        keys = torch.empty(cap, dtype=torch.int64, device=self.device)
        counts = torch.empty(cap, dtype=torch.int64, device=self.device)
        probs = torch.empty(cap, dtype=torch.float32, device=self.device)
        if self._samp is None:
            self._samp = torch.empty(2, dtype=torch.int64, device=self.device)
        info = self._samp
        if with_weights:
            weights = torch.empty(cap, dtype=torch.float64, device=self.device)
            st = self._lib.naqs_net_sample_weighted(self._h, int(n_samples), _seed64(seed), cap, keys.data_ptr(),
                                                    counts.data_ptr(), probs.data_ptr(), weights.data_ptr(), info.data_ptr(),
                                                    _stream_ptr(self.device))
        else:
            st = self._lib.naqs_net_sample(self._h, int(n_samples), _seed64(seed), cap, keys.data_ptr(),
                                           counts.data_ptr(), probs.data_ptr(), info.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_net_sample")
        m, overflow = info.tolist()
        if overflow:
            # (a look-back wait that ran out also ends the call through the overflow flag: that is an error, not a big tree)
            _lib.check(self._lib.naqs_net_check(self._h), "naqs_net_sample")
            raise MaxBatchSizeExceededError
        out = (keys[:m], counts[:m], probs[:m]) + ((weights[:m],) if with_weights else ())
        if 4 * m < cap and cap > (1 << 16):
            # a view keeps its whole cap-sized buffer alive (28 B x cap: 117 MB at the evaluation path's cap of 2^22) for as
            # long as the caller holds the result; the training path (cap = n_unq_samples_max) keeps its views
            out = tuple(t.clone() for t in out)
        return out

    @torch.no_grad()
    def sample_forward_local_energy(self, ham, n_samples, seed, max_unique):
        """``sample(with_weights=True)`` and ``forward_saved_with_local_energy`` of the sampled table in ONE library call
        (``naqs_vmc_sample_forward_eloc``): the host synchronisation that learns M happens inside the library, directly
        followed by the forward / E_loc launches, instead of a return to the interpreter in between (the GPU idles for
        that long).  -> (keys, counts, probs, weights, (log psi, saved token, E_loc, sums))."""
        from .nade import MaxBatchSizeExceededError
        cap = int(max_unique)
        dev = self.device
        keys = torch.empty(cap, dtype=torch.int64, device=dev)
        counts = torch.empty(cap, dtype=torch.int64, device=dev)
        probs = torch.empty(cap, dtype=torch.float32, device=dev)
        weights = torch.empty(cap, dtype=torch.float64, device=dev)
        log_psi = torch.empty((cap, 2), dtype=torch.float32, device=dev)
        eloc = torch.empty((cap, 2), dtype=torch.float64, device=dev)
        sums = torch.empty(4, dtype=torch.float64, device=dev)
        if self._samp is None:
            self._samp = torch.empty(2, dtype=torch.int64, device=dev)
        info_host = (ctypes.c_int64 * 2)(0, 0)
        st = self._lib.naqs_vmc_sample_forward_eloc(self._h, ham._h, int(n_samples), _seed64(seed), cap, keys.data_ptr(),
                                                    counts.data_ptr(), probs.data_ptr(), weights.data_ptr(), log_psi.data_ptr(),
                                                    eloc.data_ptr(), sums.data_ptr(), self._samp.data_ptr(), info_host,
                                                    _stream_ptr(dev))
        _lib.check(st, "naqs_vmc_sample_forward_eloc")
        m, overflow = int(info_host[0]), int(info_host[1])
        if overflow:
            raise MaxBatchSizeExceededError
        k = keys[:m]
        return k, counts[:m], probs[:m], weights[:m], (log_psi[:m], (k, None, None), eloc[:m], sums)

    @torch.no_grad()
    def vmc_step(self, ham, n_samples, seed, max_unique, m_lo, m_hi, adam=None, keys_out=None):
        """One whole VMC training step as ONE library call (``naqs_vmc_step``): sampling, the host's look at (M, overflow),
        forward + E_loc, loss gradient + backward, Adam on the flat parameter vector and the re-pack of the kernels' weight
        layouts — the interpreter is not on the GPU's critical path between the first and the last launch of the step.
        ``adam``: a ``FlatAdam`` whose flat vector is this network's (its step counter is advanced here), or None to stop
        after the backward pass (gradients in ``self._grad_flat``).  The step is abandoned after sampling when the tree
        overflowed or M is outside [m_lo, m_hi].  -> (taken, M, overflow, (keys, counts, probs, weights, log psi, E_loc,
        sums, g, ev)) — the tensors are views of length M (None when not taken)."""
        cap = int(max_unique)
        dev = self.device
        # keys_out: where the sampler writes the keys (int64 [>= cap], contiguous; e.g. the caller's tracking buffer)
        keys = keys_out if keys_out is not None else torch.empty(cap, dtype=torch.int64, device=dev)
        if keys.dtype != torch.int64 or keys.numel() < cap or not keys.is_contiguous():
            raise ValueError("vmc_step: keys_out must be a contiguous int64 tensor of at least max_unique elements")
        counts, probs, weights, log_psi, eloc, g = self._table_buffers(cap)
        # what the optimiser keeps across steps are the two device scalars (<E>, Var), which therefore get fresh storage
        # every step (the cap-sized outputs are only valid until the next step of this handle)
        small = torch.empty(6, dtype=torch.float64, device=dev)
        sums, ev = small[:4], small[4:]
        info = (ctypes.c_int64 * 3)(0, 0, 0)
        ptrs, hyper, t = self._adam_args(adam, "vmc_step") if adam is not None else ((None, None, None), (0.0,) * 5, 0)
        st = self._lib.naqs_vmc_step(self._h, ham._h, int(n_samples), _seed64(seed), cap, int(m_lo), int(m_hi),
                                     keys.data_ptr(), counts.data_ptr(), probs.data_ptr(), weights.data_ptr(), log_psi.data_ptr(),
                                     eloc.data_ptr(), sums.data_ptr(), g.data_ptr(), ev.data_ptr(), self._ensure_grad_flat().data_ptr(),
                                     *ptrs, *hyper, t, info, _stream_ptr(dev))
        _lib.check(st, "naqs_vmc_step")
        m, overflow, taken = int(info[0]), bool(info[1]), bool(info[2])
        if not taken:
            return False, m, overflow, None
        if adam is not None:
            self._adam_stepped(adam, t)
        return True, m, False, (keys[:m], counts[:m], probs[:m], weights[:m], log_psi[:m], eloc[:m], sums, g[:m], ev)

    @torch.no_grad()
    def vmc_run(self, ham, n_steps, adam, n_samples, n_samples_max, n_unq_min, n_unq_max, seed_base, sample_calls, ring=None, ring_off=0):
        """``n_steps`` training steps in ONE library call (``naqs_vmc_run``): the loop of ``PartialSamplingOptimizer.run``
        with get_samples' adaptive sample count in C.  ``ring``: the optimiser's tracking buffer (int64; the keys of step i go to
        ``ring[off:off + M]``) or None.  -> dict(steps, stop_reason, error [the NaqsError of a failed call, for the caller to raise
        once it has booked the ``steps`` that did finish; None otherwise], events [(step, n_unique, overflow, action, n_samples)],
        n_samples, sample_calls, ring_off, M [steps], ns [steps], t [steps], ev [steps, 2], sums [steps, 4], and the last step's
        table views keys / counts / probs / weights / log_psi / eloc / g)."""
        dev, cap = self.device, int(n_unq_max)
        counts, probs, weights, log_psi, eloc, g = self._table_buffers(cap)
        if ring is None:
            kb = getattr(self, "_run_keys", None)
            if kb is None or kb.numel() < cap:
                kb = self._run_keys = torch.empty(cap, dtype=torch.int64, device=dev)
            keys_buf, ring_elems = kb, 0
        else:
            if ring.dtype != torch.int64 or not ring.is_contiguous() or ring.numel() < cap:
                raise ValueError("vmc_run: the tracking buffer must be a contiguous int64 tensor of at least max_unique elements")
            keys_buf, ring_elems = ring, ring.numel()
        n = int(n_steps)
        ev = torch.empty((max(n, 1), 2), dtype=torch.float64, device=dev)
        sums = torch.empty((max(n, 1), 4), dtype=torch.float64, device=dev)
        m_log, ns_log, t_log = (ctypes.c_int64 * max(n, 1))(), (ctypes.c_int64 * max(n, 1))(), (ctypes.c_double * max(n, 1))()
        ev_cap = 64 + 4 * n
        events = (_lib.VmcEvent * ev_cap)()
        ptrs, hyper, t_next = self._adam_args(adam, "vmc_run")
        a = _lib.VmcRunArgs()
        a.n_samples, a.n_samples_max = int(n_samples), int(n_samples_max)
        a.n_unq_samples_min, a.n_unq_samples_max = int(n_unq_min), cap
        a.seed_base, a.sample_calls = _seed64(seed_base), int(sample_calls)
        a.param_dev, a.exp_avg_dev, a.exp_avg_sq_dev = ptrs
        a.grad_dev = self._ensure_grad_flat().data_ptr()
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = hyper
        a.adam_step = int(t_next) - 1                      # (the steps done so far: the library counts on from here)
        a.keys_dev, a.ring_elems, a.ring_off = keys_buf.data_ptr(), int(ring_elems), int(ring_off)
        a.counts_dev, a.probs_dev, a.weights_dev = counts.data_ptr(), probs.data_ptr(), weights.data_ptr()
        a.logpsi_dev, a.eloc_dev, a.g_dev = log_psi.data_ptr(), eloc.data_ptr(), g.data_ptr()
        a.ev_log_dev, a.sums_log_dev = ev.data_ptr(), sums.data_ptr()
        a.m_log_host, a.ns_log_host, a.t_log_host = m_log, ns_log, t_log
        a.events, a.events_cap = events, ev_cap
        st = self._lib.naqs_vmc_run(self._h, ham._h, n, ctypes.byref(a), _stream_ptr(dev))
        # A failure part-way through (a bounded device wait expiring, a HIP error at step k) leaves k finished steps behind:
        # k Adam updates are applied and the counters in `a` have advanced.  They are copied back below like a good run's, and
        # the error travels in the result ("error") so that the caller books the finished steps BEFORE it raises.
        error = None
        try:
            _lib.check(st, "naqs_vmc_run")
        except _lib.NaqsError as exc:
            error = exc
        done = int(a.steps_done)
        if done:
            self._adam_stepped(adam, int(a.adam_step))
        m_last = int(m_log[done - 1]) if done else 0
        k0 = int(a.last_keys_off)
        return dict(steps=done, stop_reason=int(a.stop_reason), error=error,
                    events=[(int(e.step), int(e.n_unique), bool(e.overflow), int(e.action), int(e.n_samples)) for e in events[:int(a.n_events)]],
                    n_samples=int(a.n_samples), sample_calls=int(a.sample_calls), ring_off=int(a.ring_off),
                    M=[int(x) for x in m_log[:done]], ns=[int(x) for x in ns_log[:done]], t=[float(x) for x in t_log[:done]],
                    ev=ev, sums=sums, keys=keys_buf[k0:k0 + m_last], counts=counts[:m_last], probs=probs[:m_last],
                    weights=weights[:m_last], log_psi=log_psi[:m_last], eloc=eloc[:m_last], g=g[:m_last])

    # ---- the row-sharded step (world > 1): four library calls, the three collectives between them (include/naqs_hip.h) ----
    def _step_buffers(self, cap, world, keys_out=None):
        """Per-handle buffers of the sharded step, allocated once per (cap, world): the step's outputs are views of them and
        stay valid until the next step, like ``_table_buffers``' of the single process's one-call step; the flat gradient
        the step's backward writes and all-reduces is made here too."""
        key = (int(cap), int(world))
        sb = getattr(self, "_shard_bufs", None)
        if sb is None or sb["key"] != key:
            dev = self.device
            S_pad = -(-int(cap) // int(world))
            sb = self._shard_bufs = dict(
                key=key, S_pad=S_pad,
                keys=torch.empty(cap, dtype=torch.int64, device=dev), counts=torch.empty(cap, dtype=torch.int64, device=dev),
                probs=torch.empty(cap, dtype=torch.float32, device=dev), weights=torch.empty(cap, dtype=torch.float64, device=dev),
                mine=torch.zeros((S_pad, 2), dtype=torch.float32, device=dev),
                table=torch.empty((S_pad * int(world), 2), dtype=torch.float32, device=dev),
                eloc=torch.empty((S_pad, 2), dtype=torch.float64, device=dev), g=torch.empty((S_pad, 2), dtype=torch.float32, device=dev),
                ext=torch.empty(8, dtype=torch.float64, device=dev), ev=torch.empty(2, dtype=torch.float64, device=dev))
        self._ensure_grad_flat()
        return sb

    @torch.no_grad()
    def shard_sample_forward(self, n_samples, seed, max_unique, m_lo, m_hi, rank, world, keys_out=None):
        """Call 1 (``naqs_vmc_shard_sample_forward``): the sampler, the host's look at (M, overflow), and the training forward
        of this rank's rows, whose (log|psi|, phase) land at the front of the gather contribution.
        -> (taken, M, overflow, buffers)."""
        cap = int(max_unique)
        sb = self._step_buffers(cap, world)
        keys = keys_out if keys_out is not None else sb["keys"]
        if keys.dtype != torch.int64 or keys.numel() < cap or not keys.is_contiguous():
            raise ValueError("shard_sample_forward: keys_out must be a contiguous int64 tensor of at least max_unique elements")
        info = (ctypes.c_int64 * 3)(0, 0, 0)
        st = self._lib.naqs_vmc_shard_sample_forward(self._h, int(n_samples), _seed64(seed), cap, int(m_lo), int(m_hi),
                                                     int(rank), int(world), keys.data_ptr(), sb["counts"].data_ptr(),
                                                     sb["probs"].data_ptr(), sb["weights"].data_ptr(), sb["mine"].data_ptr(), info,
                                                     _stream_ptr(self.device))
        _lib.check(st, "naqs_vmc_shard_sample_forward")
        sb["keys_used"] = keys
        return bool(info[2]), int(info[0]), bool(info[1]), sb

    @torch.no_grad()
    def shard_eloc(self, ham, sb, M, rank, world):
        """Call 2 (``naqs_eloc_gathered``) on the all-gathered table: E_loc of my rows, weighted sums and the same-table proof
        -> ext8 (to be all-reduced).  -> (b, e): my row range."""
        S = -(-M // world)
        b = min(M, rank * S)
        e = min(M, b + S)
        st = self._lib.naqs_eloc_gathered(ham._h, M, sb["keys_used"].data_ptr(), sb["table"].data_ptr(), S, sb["S_pad"], b, e - b,
                                          sb["weights"][b:].data_ptr() if e > b else None, sb["eloc"].data_ptr(), sb["ext"].data_ptr(),
                                          _stream_ptr(self.device))
        _lib.check(st, "naqs_eloc_gathered")
        return b, e

    @torch.no_grad()
    def shard_backward(self, sb, b, e):
        """Call 3 (``naqs_net_train_backward_vmc``) for my rows with the all-reduced sums -> flat gradient of my shard."""
        st = self._lib.naqs_net_train_backward_vmc(self._h, e - b, sb["keys_used"][b:].data_ptr() if e > b else None,
                                                   sb["eloc"].data_ptr(), sb["weights"][b:].data_ptr() if e > b else None,
                                                   sb["ext"].data_ptr(), sb["g"].data_ptr(), sb["ev"].data_ptr(),
                                                   self._grad_flat.data_ptr(), _stream_ptr(self.device))
        _lib.check(st, "naqs_net_train_backward_vmc")

    @torch.no_grad()
    def shard_update(self, adam):
        """Call 4 (``naqs_vmc_shard_update``): Adam on the flat parameter vector with the all-reduced gradient + re-pack."""
        ptrs, hyper, t = self._adam_args(adam, "shard_update")
        st = self._lib.naqs_vmc_shard_update(self._h, self._grad_flat.data_ptr(), *ptrs, *hyper, t, _stream_ptr(self.device))
        _lib.check(st, "naqs_vmc_shard_update")
        self._adam_stepped(adam, t)

    def prof_enable(self, n, stride=1):
        _lib.check(self._lib.naqs_net_prof_enable(self._h, int(n)), "naqs_net_prof_enable")
        _lib.check(self._lib.naqs_net_prof_stride(self._h, int(stride)), "naqs_net_prof_stride")

    def prof_read(self):
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        _lib.check(self._lib.naqs_net_prof_read(self._h, ctypes.byref(ms), ctypes.byref(n)), "naqs_net_prof_read")
        return ms.value, n.value

    def last_kernel(self):
        """Name (with template arguments) of the kernel the most recent log-psi call launched, followed by the amplitude or
        aggregate-phase launches that went with it (" + amp_mfma_kernel<4>"); measurement aid and dispatch check."""
        buf = ctypes.create_string_buffer(256)
        _lib.check(self._lib.naqs_net_last_kernel(self._h, buf, 256), "naqs_net_last_kernel")
        return buf.value.decode()

    def share_device(self, on=None):
        """Two runs per GPU (the farm's `--per-gpu 2`): this handle's sampler calls take turns with those of the device's other
        sharing handles (`naqs_net_share_device`; default NAQS_SHARED_GPU when the handle was created).  `on=None` only reads.
        -> sampler calls so far that had to wait for another handle's turn to end."""
        turns = ctypes.c_int64(0)
        _lib.check(self._lib.naqs_net_share_device(self._h, -1 if on is None else int(bool(on)), ctypes.byref(turns)),
                   "naqs_net_share_device")
        return turns.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.naqs_net_destroy(self._h)
            self._h = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
