"""Approximate MPC with do_mpc.approximateMPC's user surface: a small feed-forward network trained on solved MPC problems replaces
the solve in the loop; the step is batched on the GPU.

Reference surface mirrored here (/root/reference/do_mpc/approximateMPC/_ampc.py, _trainer.py, _ampcsettings.py):
`ApproximateMPCSettings`, `TrainerSettings`, `TrainerSchedulerSettings`, `FeedforwardNN` (the reference's `state_dict` keys
`layers.<2 i>.weight / .bias`, activation layers on the odd slots: a `.pth` of either side loads on the other), `ApproxMPC(mpc)`
with `settings`, `setup()`, `make_step(x0, u_prev=None, clip_to_bounds=True)`, `predict`, `scale_inputs`, `rescale_outputs`,
`clip_control_actions`, `save_to_state_dict`, `load_from_state_dict`, the iterated `x0` / `u0`, `step_return_type`, and
`Trainer(approx_mpc)` with `settings`, `scheduler_settings`, `setup()`, `default_training()` and the reference's steps.  The
trainer reads `<data_dir>/<name>/data_<name>_opt.pkl`, the file do_mpc_amd.sampling.AMPCSampler writes.

Underneath, `make_step` - scale the input [x; u_prev] by its bounds box, the network in float32, rescale, clip - is ONE launch of
csrc/dompc_ampc.hip behind the C ABI `dompc_ampc_*` (include/dompc_ipm.h) for a whole batch: `make_step_batch` on host arrays,
`make_step_batch_device` on device pointers; `make_step` is the batch of one.  The code object belongs to the network's SHAPE; the
weights are packed and uploaded before a step whenever a parameter changed (an optimiser step, `load_from_state_dict`).
Training is PyTorch (Adam, mse_loss, ReduceLROnPlateau) and `predict` is the plain torch forward of `self.net`.

Additions to the reference's surface: `jacobian_batch` / `jacobian_batch_device` - u and the network's own Jacobian du/dx, du/du_prev
for a batch in one launch of the second kernel of the same code object (`dompc_ampc_jacobian_batch*`) - and Sobolev training:
`TrainerSettings.sobolev_weight` > 0 also fits that Jacobian to the MPC sensitivities the sampler stored (`du0dx0`, `du0du_prev`),
`Trainer.sensitivity_error()` measures it against them.

Two behaviours of the reference are deliberately NOT copied:
  * `setup()` does not call `torch.set_default_device`: a process-wide side effect that would change every other torch user in
    the process.  The trainer moves the network and its data to `cuda:<gpu_index>` itself when a device is there.
  * `setup()` does not print the module.
One quirk of the reference IS kept, since the `state_dict` has to match: with `n_hidden_layers = 0` the network is the one layer
Linear(n_in, n_neurons) followed by `act_fn`; it is usable only with `n_neurons` = number of plant inputs.

There is no CPU fallback: without a HIP device `make_step*` raises.  Limits of the kernel: n_in <= 64, n_out <= 32,
n_neurons <= 128, n_hidden_layers <= 8; larger networks are refused by name in `setup()`.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import pickle as pkl
import warnings
from dataclasses import dataclass
from pathlib import Path
from statistics import fmean
from typing import Optional

import numpy as np
import torch

from . import _native, build, lowering


@dataclass
class ApproximateMPCSettings:
    """_ampcsettings.py:28-57; `gpu_index` as the other settings classes here"""
    n_hidden_layers: int = 3
    n_neurons: int = 50
    act_fn: str = "tanh"
    output_act_fn: str = "linear"
    device: str = "auto"
    scaling: bool = True
    lbx: list = None
    ubx: list = None
    lbu: list = None
    ubu: list = None
    gpu_index: int = 0


@dataclass
class TrainerSettings:
    """_ampcsettings.py:123-180"""
    dataset_name: str = None
    n_epochs: int = None
    data_dir: str = os.path.join(".", "sampling")
    results_dir: str = os.path.join(".", "training")
    scheduler_flag: bool = False
    val: float = 0.2
    batch_size: int = 1000
    shuffle: bool = True
    learning_rate: float = 1e-3
    show_fig: bool = False
    save_fig: bool = False
    save_history: bool = False
    print_frequency: int = 10
    gpu_index: int = 0
    sobolev_weight: float = 0.0            # (addition) > 0: the loss also fits the network's Jacobian to du0dx0 / du0du_prev of the data file

    def check_for_mandatory_settings(self):
        if self.dataset_name is None:
            raise ValueError("The dataset name must be provided")
        if self.n_epochs is None:
            raise ValueError("A number of epochs must be set")


@dataclass
class TrainerSchedulerSettings:
    """_ampcsettings.py:183-215"""
    mode: str = "min"
    factor: float = 0.1
    patience: float = 10
    threshold: float = 1e-4
    threshold_mode: str = "rel"
    cooldown: float = 2
    min_lr: float = 1e-7
    eps: float = 1e-8
    gpu_index: int = 0


# activation names of the settings -> torch layers ("linear": no layer, for the output only)
_ACTIVATION_LAYERS = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "leaky_relu": torch.nn.LeakyReLU, "sigmoid": torch.nn.Sigmoid}


def _layer_plan(n_in, n_out, n_hidden_layers, n_neurons, act_fn, output_act_fn):
    """[(inputs, outputs, activation name or None)] of the linear layers.  The reference's rule, which fixes the `state_dict`: the
    first layer always maps to n_neurons and ends in act_fn - so WITHOUT a hidden layer it is the whole network and output_act_fn is
    not used -; otherwise the last layer maps to n_out and ends in output_act_fn, "linear" meaning no activation layer."""
    if n_hidden_layers == 0:
        return [(n_in, n_neurons, act_fn)]
    hidden = [(n_in, n_neurons, act_fn)] + [(n_neurons, n_neurons, act_fn)] * (n_hidden_layers - 1)
    return hidden + [(n_neurons, n_out, None if output_act_fn == "linear" else output_act_fn)]


class FeedforwardNN(torch.nn.Module):
    """The network of the reference's FeedforwardNN by its interface: `layers` is a ModuleList with the linear layers on the even slots
    and the activation layers on the odd ones, so the `state_dict` keys are `layers.0.weight`, `layers.0.bias`, `layers.2.weight`, ..."""

    def __init__(self, n_in, n_out, n_hidden_layers, n_neurons, act_fn, output_act_fn):
        super().__init__()
        assert n_hidden_layers >= 0, "Number of hidden layers must be >= 0."
        self.n_in, self.n_out, self.n_layers, self.n_neurons = n_in, n_out, n_hidden_layers + 1, n_neurons
        self.act_fn, self.output_act_fn = act_fn, output_act_fn
        modules = []
        for inputs, outputs, act in _layer_plan(n_in, n_out, n_hidden_layers, n_neurons, act_fn, output_act_fn):
            modules.append(torch.nn.Linear(inputs, outputs))
            if act is not None:
                if act not in _ACTIVATION_LAYERS:
                    raise ValueError("Activation function not implemented.")
                modules.append(_ACTIVATION_LAYERS[act]())
        self.layers = torch.nn.ModuleList(modules)

    def forward(self, x):
        for module in self.layers:
            x = module(x)
        return x


def network_jacobian(net: FeedforwardNN, xs):
    """(net(xs), d net / d xs [B][n_out][n_in]) by the tangent recursion over `net.layers`, T <- diag(act'(a)) W T with the activation's
    derivative formed from its output a - the arithmetic of csrc/dompc_ampc.hip:jac32 -, in torch operations, so that autograd reaches
    the weights through both results"""
    h, T = xs, None
    for module in net.layers:
        if isinstance(module, torch.nn.Linear):
            h = module(h)
            T = module.weight if T is None else module.weight @ T
            continue
        h = module(h)
        if isinstance(module, torch.nn.Tanh):
            d = 1.0 - h * h
        elif isinstance(module, torch.nn.Sigmoid):
            d = h * (1.0 - h)
        elif isinstance(module, torch.nn.ReLU):
            d = (h > 0).to(h.dtype)
        elif isinstance(module, torch.nn.LeakyReLU):
            d = torch.where(h > 0, 1.0, module.negative_slope).to(h.dtype)
        else:
            raise ValueError("Activation function not implemented.")
        T = d.unsqueeze(-1) * T
    return h, (T if T.dim() == 3 else T.expand(xs.shape[0], *T.shape))


# ---------------------------------------------------------------------------------------------------------------------- native side
class AMPCDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_in", "n_out", "n_hidden_layers", "n_neurons", "act", "out_act", "scaling", "nx")] + \
               [("code_object_path", C.c_char_p), ("model_hash", C.c_char_p), ("device", C.c_int32)]


def _bind(lib_path: str) -> C.CDLL:
    lib = C.CDLL(lib_path)
    vp = C.c_void_p
    lib.dompc_ampc_create.argtypes = [C.POINTER(AMPCDesc), C.POINTER(vp)]
    lib.dompc_ampc_create.restype = C.c_int
    lib.dompc_ampc_destroy.argtypes = [vp]
    lib.dompc_ampc_last_error.argtypes = [vp]
    lib.dompc_ampc_last_error.restype = C.c_char_p
    lib.dompc_ampc_packed_size.argtypes = [vp]
    lib.dompc_ampc_packed_size.restype = C.c_int64
    lib.dompc_ampc_set_weights.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp]
    lib.dompc_ampc_set_weights.restype = C.c_int
    lib.dompc_ampc_device_weights.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.dompc_ampc_device_weights.restype = C.c_int
    lib.dompc_ampc_step_batch.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32]
    lib.dompc_ampc_step_batch.restype = C.c_int
    lib.dompc_ampc_step_batch_device.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, vp]
    lib.dompc_ampc_step_batch_device.restype = C.c_int
    lib.dompc_ampc_jacobian_batch.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, C.c_int32]
    lib.dompc_ampc_jacobian_batch.restype = C.c_int
    lib.dompc_ampc_jacobian_batch_device.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, C.c_int32, vp]
    lib.dompc_ampc_jacobian_batch_device.restype = C.c_int
    return lib


def _pack_layer(W: np.ndarray, b: np.ndarray) -> np.ndarray:
    """one layer in the operand order of csrc/dompc_ampc.hip: [out tile][in tile][step g][lane] = W[32 to + (lane & 31)]
    [32 tk + 8 (g >> 2) + 4 (lane >> 5) + (g & 3)] - the column that register g of the lane's half holds in the accumulator tile of
    the layer before - then the bias, both padded with zeros to whole tiles (a padded neuron is inert: its row gives
    act(0), and its column in the next layer is zero)"""
    n_out, n_in = W.shape
    to, tk = (n_out + 31) // 32, (n_in + 31) // 32
    Wp = np.zeros((32 * to, 32 * tk), dtype=np.float32)
    Wp[:n_out, :n_in] = W
    bp = np.zeros(32 * to, dtype=np.float32)
    bp[:n_out] = b
    lane, g = np.arange(64)[None, :], np.arange(16)[:, None]
    col = 8 * (g >> 2) + 4 * (lane >> 5) + (g & 3)                     # [16][64]
    row = np.broadcast_to(lane & 31, col.shape)
    blocks = [Wp[32 * o + row, 32 * k + col] for o in range(to) for k in range(tk)]
    return np.concatenate([np.stack(blocks).ravel(), bp])


def pack_weights(state_dict) -> np.ndarray:
    """the packed float32 weights of a FeedforwardNN `state_dict` (`layers.<2 i>.weight / .bias`), layer after layer"""
    idx = sorted({int(k.split(".")[1]) for k in state_dict if k.endswith(".weight")})
    t = lambda v: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)).astype(np.float32)      # noqa: E731
    return np.ascontiguousarray(np.concatenate([_pack_layer(t(state_dict[f"layers.{i}.weight"]), t(state_dict[f"layers.{i}.bias"]))
                                                for i in idx]))


def _flat(v) -> np.ndarray:
    if hasattr(v, "master"):
        v = v.master
    elif hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    elif hasattr(v, "arr"):
        v = v.arr
    return np.asarray(v, dtype=np.float64).reshape(-1)


class ApproxMPC(torch.nn.Module):
    def __init__(self, mpc):
        super().__init__()
        self._settings = ApproximateMPCSettings()
        self.mpc = mpc
        st = self._settings
        st.lbx, st.ubx = _flat(mpc._x_lb).reshape(-1, 1).copy(), _flat(mpc._x_ub).reshape(-1, 1).copy()
        st.lbu, st.ubu = _flat(mpc._u_lb).reshape(-1, 1).copy(), _flat(mpc._u_ub).reshape(-1, 1).copy()
        self.flags = {"setup": False}
        self._native = _native.Native("ampc", _bind, build.ampc_code_object)
        self._uploaded = None             # what the handle's weights were packed from
        self._epoch = 0                   # bumped by load_from_state_dict / the trainer

    @property
    def settings(self):
        return self._settings

    @settings.setter
    def settings(self, val):
        warnings.warn("Cannot change the settings attribute")

    _lib = property(lambda self: self._native.lib)     # the bound library and the native handle (None before first use / after close)
    _h = property(lambda self: self._native.h)

    # ------------------------------------------------------------------ setup
    def setup(self, _lib_path=None, _code_object: Optional[str] = None) -> None:
        """Builds the network and the scaling from the bounds; the settings are final from here on.  With n_hidden_layers = 0 the
        network is one layer ending in act_fn and settings.output_act_fn is not used (the reference's layer rule).  TEST-ONLY: `_lib_path` (a path, or a callable (header, hash) -> path)
        with `_code_object=""` selects the host emulation of the kernel."""
        assert self.flags["setup"] is False, "Setup can only be once."
        st, m = self.settings, self.mpc.model
        self._native = _native.Native("ampc", _bind, build.ampc_code_object, _lib_path, _code_object)
        self.rterm = bool(self.mpc.flags["set_rterm"])
        n_in = m.n_x + m.n_u if self.rterm else m.n_x
        self.net = FeedforwardNN(n_in=n_in, n_out=m.n_u, n_hidden_layers=st.n_hidden_layers, n_neurons=st.n_neurons, act_fn=st.act_fn,
                                 output_act_fn=st.output_act_fn)
        # the kernel's shape: refuses a network beyond its limits, naming the limit
        self.generated_header = lowering.lower_ampc(n_in, m.n_u, st.n_hidden_layers, st.n_neurons, st.act_fn, st.output_act_fn, st.scaling)
        self.model_hash = self.generated_header.rsplit('AMPC_MODEL_HASH "', 1)[1].split('"')[0]
        self.torch_data_type = torch.float32
        self.step_return_type = "numpy"   # "torch" or "numpy"
        self.x0 = self.mpc.x0
        self.u0 = self.mpc.u0
        inf = lambda v: bool(np.any(np.isinf(_flat(v))))      # noqa: E731
        assert inf(st.lbx) is False, "There are missing lower bounds for state variables that are required for clipping and scaling."
        assert inf(st.ubx) is False, "There are missing upper bounds for state variables that are required for clipping and scaling."
        assert inf(st.lbu) is False, "There are missing lower bounds for input variables that are required for clipping and scaling."
        assert inf(st.ubu) is False, "There are missing upper bounds for input variables that are required for clipping and scaling."
        self.flags["setup"] = True
        self.set_shift_values()
        self._params = list(self.net.parameters())

    def _box(self):
        """(lb_in, ub_in, lbu, ubu) as flat float64 arrays"""
        st = self.settings
        lbx, ubx, lbu, ubu = (_flat(v) for v in (st.lbx, st.ubx, st.lbu, st.ubu))
        if self.rterm:
            return np.concatenate((lbx, lbu)), np.concatenate((ubx, ubu)), lbu, ubu
        return lbx, ubx, lbu, ubu

    def set_shift_values(self) -> None:
        lb, ub, lbu, ubu = self._box()
        self.x_shift = torch.tensor(lb.reshape(1, -1))
        self.x_range = torch.tensor((ub - lb).reshape(1, -1))
        self.y_shift = torch.tensor(lbu.reshape(1, -1))
        self.y_range = torch.tensor((ubu - lbu).reshape(1, -1))

    # ------------------------------------------------------------------ the torch side (training, predict)
    def forward(self, x):
        return self.net(x)

    def scale_inputs(self, x):
        x_scaled = (x - self.x_shift.to(x.device)) / self.x_range.to(x.device)
        return x_scaled.type(self.torch_data_type)

    def rescale_outputs(self, y_scaled):
        return y_scaled * self.y_range.to(y_scaled.device) + self.y_shift.to(y_scaled.device)

    def clip_control_actions(self, y):
        """y clamped to [lbu, ubu]: first from below, then from above"""
        st = self.settings
        if st.lbu is None and st.ubu is None:
            raise ValueError("No output constraints defined. Clipping not possible.")
        bound = lambda v: None if v is None else torch.as_tensor(_flat(v).reshape(1, -1), dtype=y.dtype, device=y.device)      # noqa: E731
        return torch.clamp(y, min=bound(st.lbu), max=bound(st.ubu))

    @torch.no_grad()
    def predict(self, x_batch):
        return self.net(x_batch)

    def save_to_state_dict(self, directory="approx_mpc.pth"):
        torch.save(self.net.state_dict(), directory)

    def load_from_state_dict(self, directory="approx_mpc.pth"):
        self.net.load_state_dict(torch.load(directory, weights_only=True))
        self._epoch += 1

    # ------------------------------------------------------------------ the native step
    def _handle(self):
        """the runtime handle (created on first use) with the CURRENT weights: packed and uploaded again when a parameter's version
        counter, its storage or the bounds changed since the last upload"""
        assert self.flags["setup"] is True, "MPC was not setup yet. Please call ApproxMPC.setup()."
        st, m = self.settings, self.mpc.model
        if self._h is None:
            code_object = self._native.load(self.generated_header, self.model_hash)
            desc = AMPCDesc(**self.shape_fields(), nx=m.n_x, code_object_path=code_object.encode(),
                            model_hash=self.model_hash.encode(), device=st.gpu_index)
            self._native.create(desc)
        # (the box was fixed by setup(): settings cannot change afterwards; only the parameters are looked at per step)
        key = (self._epoch, sum(p._version for p in self._params), tuple(p.data_ptr() for p in self._params))
        if key != self._uploaded:
            packed = pack_weights(self.net.state_dict())
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
            box = [np.ascontiguousarray(a, dtype=np.float64) for a in self._box()]
            self._check(self._lib.dompc_ampc_set_weights(self._h, ptr(packed), packed.size, *[ptr(a) for a in box]))
            self._uploaded = key
        return self._h

    def shape_fields(self) -> dict:
        """the network's shape as the native descriptions name it (dompc_ampc_desc, dompc_plant_ampc_loop_desc)"""
        st, act = self.settings, lowering.AMPC_ACTIVATIONS
        return dict(n_in=self.net.n_in, n_out=self.mpc.model.n_u, n_hidden_layers=st.n_hidden_layers, n_neurons=st.n_neurons,
                    act=act[st.act_fn], out_act=act[st.act_fn if st.n_hidden_layers == 0 else st.output_act_fn],
                    scaling=1 if st.scaling else 0)

    def device_weights(self):
        """(w, par): the device addresses of the handle's packed weights and of its scaling and bounds, holding the CURRENT weights
        (`dompc_ampc_device_weights`) - what the fused loop of `Simulator.rollout_ampc_device` reads"""
        h = self._handle()
        w, par = C.c_void_p(), C.c_void_p()
        self._check(self._lib.dompc_ampc_device_weights(h, C.byref(w), C.byref(par)))
        return w.value, par.value

    def _check(self, rc):
        self._native.check(rc)

    def close(self):
        self._native.close()
        self._uploaded = None

    def _host_inputs(self, X, U_prev, who):
        """(X [B][nx], U_prev [B][nu] or None) as contiguous float64 arrays"""
        m = self.mpc.model
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64)).reshape(-1, m.n_x)
        up = None
        if self.rterm:
            if U_prev is None:
                raise ValueError(f"{who}: the controller has an rterm, the network input is [x; u_prev]: U_prev is required")
            up = np.ascontiguousarray(np.asarray(U_prev, dtype=np.float64)).reshape(X.shape[0], m.n_u)
        return X, up

    def make_step_batch(self, X, U_prev=None, clip_to_bounds=True) -> np.ndarray:
        """one step for B samples in one launch: X [B][nx] (and U_prev [B][nu] when the controller has an rterm) -> U [B][nu], float64"""
        h = self._handle()
        X, up = self._host_inputs(X, U_prev, "make_step_batch")
        B = X.shape[0]
        U = np.empty((B, self.mpc.model.n_u))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731
        self._check(self._lib.dompc_ampc_step_batch(h, B, ptr(X), ptr(up), ptr(U), 1 if clip_to_bounds else 0))
        return U

    def make_step_batch_device(self, B, X_ptr, U_prev_ptr, U_out_ptr, stream=0, clip_to_bounds=True) -> None:
        """make_step_batch on raw device addresses (ints, e.g. torch tensor .data_ptr()) of float64 arrays [B][nx], [B][nu] (0 without
        an rterm) and [B][nu]; asynchronous on `stream`"""
        h = self._handle()
        self._check(self._lib.dompc_ampc_step_batch_device(
            h, int(B), C.c_void_p(int(X_ptr)), C.c_void_p(int(U_prev_ptr) if U_prev_ptr else None), C.c_void_p(int(U_out_ptr)),
            1 if clip_to_bounds else 0, C.c_void_p(int(stream) if stream else None)))

    def jacobian_batch(self, X, U_prev=None, clip_to_bounds=False) -> dict:
        """the network's own Jacobian for B samples in one launch (dompc_ampc_jac_kernel: forward mode in float32): {"u": [B][nu] as
        make_step_batch gives it, "du_dx": [B][nu][nx], "du_du_prev": [B][nu][nu] or None without an rterm}, float64, in physical
        units like the sampler's du0dx0 / du0du_prev.  With clip_to_bounds the row of an output that lay beyond a bound is zero."""
        h = self._handle()
        m = self.mpc.model
        X, up = self._host_inputs(X, U_prev, "jacobian_batch")
        B = X.shape[0]
        out = {"u": np.empty((B, m.n_u)), "du_dx": np.empty((B, m.n_u, m.n_x)), "du_du_prev": np.empty((B, m.n_u, m.n_u)) if self.rterm else None}
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None      # noqa: E731
        self._check(self._lib.dompc_ampc_jacobian_batch(h, B, ptr(X), ptr(up), ptr(out["u"]), ptr(out["du_dx"]), ptr(out["du_du_prev"]),
                                                        1 if clip_to_bounds else 0))
        return out

    def jacobian_batch_device(self, B, X_ptr, U_prev_ptr, U_out_ptr, dUdX_ptr, dUdUprev_ptr, stream=0, clip_to_bounds=False) -> None:
        """jacobian_batch on raw device addresses of float64 arrays [B][nx], [B][nu], [B][nu], [B][nu][nx] and [B][nu][nu] (U_prev_ptr and
        dUdUprev_ptr 0 without an rterm); asynchronous on `stream`"""
        h = self._handle()
        vp = lambda a: C.c_void_p(int(a) if a else None)      # noqa: E731
        self._check(self._lib.dompc_ampc_jacobian_batch_device(h, int(B), vp(X_ptr), vp(U_prev_ptr), vp(U_out_ptr), vp(dUdX_ptr),
                                                               vp(dUdUprev_ptr), 1 if clip_to_bounds else 0, vp(stream)))

    def make_step(self, x0, u_prev=None, clip_to_bounds=True):
        assert self.flags["setup"] == True, "MPC was not setup yet. Please call ApproxMPC.setup()."      # noqa: E712
        assert isinstance(x0, np.ndarray), "x0 must be a numpy array"
        assert isinstance(u_prev, (np.ndarray, type(None))), "u_prev must be a numpy array or None"
        if u_prev is not None:
            self.u0 = u_prev
        if self.step_return_type not in ("numpy", "torch"):
            raise ValueError("step_return_type must be either 'numpy' or 'torch'.")
        U = self.make_step_batch(x0.reshape(1, -1), _flat(self.u0).reshape(1, -1) if self.rterm else None, clip_to_bounds)
        self.u0 = U.reshape(-1, 1) if self.step_return_type == "numpy" else torch.from_numpy(U)      # (column / row, as the reference returns them)
        return self.u0


# ---------------------------------------------------------------------------------------------------------------------- training
def _pyplot():
    try:
        import matplotlib.pyplot as plt
    except ImportError as e:
        raise ImportError("matplotlib is required for TrainerSettings.show_fig / save_fig and is not installed") from e
    return plt


class Trainer:
    """_trainer.py: Adam on mse_loss over the (scaled) samples of `data_<name>_opt.pkl`, a random validation split, optionally
    ReduceLROnPlateau.  Runs on cuda:<gpu_index> when a device is there, otherwise on the CPU; the network stays there afterwards.

    Addition (Sobolev training): with `settings.sobolev_weight` = w > 0 the data file's MPC sensitivities du0dx0 (and du0du_prev with an
    rterm; AMPCSampler.settings.store_sensitivities) become labels of the network's Jacobian, in the network's coordinates
    Js[i][k] = J[i][k] x_range[k] / y_range[i], and the loss is mse(net(xs), us) + w mse(J_net(xs), Js), the second term over the rows
    whose labels are all finite (the sampler writes NaN where the differentiation failed).  The history then also carries the two terms
    as train_loss_u / train_loss_j / val_loss_u / val_loss_j.  With the default 0.0 nothing of this is read or computed."""

    def __init__(self, approx_mpc):
        self.approx_mpc = approx_mpc
        self._settings = TrainerSettings()
        self._sc_settings = TrainerSchedulerSettings()
        self.flags = {"setup": False}

    def setup(self):
        assert self.flags["setup"] is False, "Setup can only be once."
        self.flags.update({"setup": True})
        self._settings.check_for_mandatory_settings()
        self.device = torch.device("cuda", self._settings.gpu_index) if torch.cuda.is_available() else torch.device("cpu")
        self.approx_mpc.net.to(self.device)
        self.generator = torch.Generator()          # (the trainer's own: the split and the shuffling do not touch the global one)
        self.history = {"epoch": []}
        self._terms = []                            # (loss_u, loss_j) of the mini-batches of a Sobolev epoch

    @property
    def settings(self):
        return self._settings

    @settings.setter
    def settings(self, val):
        warnings.warn("Cannot change the settings attribute")

    @property
    def scheduler_settings(self):
        return self._sc_settings

    @scheduler_settings.setter
    def scheduler_settings(self, val):
        warnings.warn("Cannot change the scheduler_settings attribute")

    def _results(self) -> Path:
        d = Path(self.settings.results_dir).joinpath("results_" + self.settings.dataset_name)
        d.mkdir(parents=True, exist_ok=True)
        return d

    def scale_dataset(self, x, u0):
        assert self.flags["setup"] == True, "MPC was not setup yet. Please call Trainer.setup()."      # noqa: E712
        a = self.approx_mpc
        x_scaled = (x - a.x_shift.to(x.device)) / a.x_range.to(x.device)
        u0_scaled = (u0 - a.y_shift.to(u0.device)) / a.y_range.to(u0.device)
        return x_scaled.type(a.torch_data_type), u0_scaled.type(a.torch_data_type)

    def _scaled_columns(self, dataset, sensitivities, source="the data"):
        """(xs, us) of a data table in the network's coordinates and data type and, on request, the Jacobian labels Js [N][n_u][n_in]"""
        a = self.approx_mpc
        m, rterm = a.mpc.model, a.mpc.flags["set_rterm"]
        col = lambda key, *n: torch.tensor(np.stack([np.asarray(v, dtype=float).reshape(-1) for v in dataset[key]]),      # noqa: E731
                                           dtype=a.torch_data_type).reshape(-1, *n)
        x0, u0 = col("x0", m.n_x), col("u0", m.n_u)
        x = torch.cat((x0, col("u_prev", m.n_u)), dim=1) if rterm else x0
        if a.settings.scaling:
            x_scaled, u0_scaled = self.scale_dataset(x, u0)
        else:
            x_scaled, u0_scaled = x, u0
        if not sensitivities:
            return x_scaled, u0_scaled
        for key in ["du0dx0"] + (["du0du_prev"] if rterm else []):
            if key not in dataset:
                raise ValueError(f"TrainerSettings.sobolev_weight > 0 needs the column {key} in {source}: sample with "
                                 "AMPCSampler.settings.store_sensitivities = True")
        J = col("du0dx0", m.n_u, m.n_x)
        if rterm:
            J = torch.cat((J, col("du0du_prev", m.n_u, m.n_u)), dim=2)
        if a.settings.scaling:
            J = (J * a.x_range.reshape(1, 1, -1) / a.y_range.reshape(1, -1, 1)).type(a.torch_data_type)
        return x_scaled, u0_scaled, J

    def load_data(self):
        assert self.flags["setup"] == True, "MPC was not setup yet. Please call Trainer.setup()."      # noqa: E712
        st, sc, a = self.settings, self.scheduler_settings, self.approx_mpc
        self.hyperparameters = {
            "data_dir": st.data_dir, "dataset_name": st.dataset_name, "scheduler_flag": st.scheduler_flag, "lr_reduce_factor": sc.factor,
            "lr_scheduler_patience": sc.patience, "lr_scheduler_cooldown": sc.cooldown, "min_lr": sc.min_lr, "val": st.val,
            "batch_size": st.batch_size, "shuffle": st.shuffle, "learning_rate": st.learning_rate}
        with open(self._results().joinpath("hyperparameters.json"), "w") as f:
            json.dump(self.hyperparameters, f, indent=4)
        data_dir = Path(st.data_dir).joinpath(st.dataset_name).joinpath("data_" + st.dataset_name + "_opt.pkl")
        print(f"Path from trainer to sampled files\n {data_dir}")
        with open(data_dir, "rb") as f:
            dataset = pkl.load(f)
        tensors = [t.to(self.device) for t in self._scaled_columns(dataset, st.sobolev_weight > 0, data_dir)]
        from torch.utils.data import DataLoader, TensorDataset, random_split
        data = TensorDataset(*tensors)
        training_data, val_data = random_split(data, [1 - st.val, st.val], generator=self.generator)
        train_dataloader = DataLoader(training_data, batch_size=st.batch_size, shuffle=st.shuffle, generator=self.generator)
        test_dataloader = DataLoader(val_data, batch_size=st.batch_size, shuffle=st.shuffle, generator=self.generator)
        optimizer = torch.optim.Adam(a.net.parameters(), lr=st.learning_rate)
        if st.scheduler_flag:
            self.lr_scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(
                optimizer, mode=sc.mode, factor=sc.factor, patience=sc.patience, threshold=sc.threshold, threshold_mode=sc.threshold_mode,
                cooldown=sc.cooldown, min_lr=sc.min_lr * 0.1, eps=sc.eps)
        return train_dataloader, test_dataloader, optimizer

    def log_value(self, val, key):
        """append one scalar to history[key]"""
        val = val.item() if torch.is_tensor(val) else val
        assert isinstance(val, (int, float)), "Value must be a scalar."
        self.history.setdefault(key, []).append(val)

    def print_last_entry(self, keys=None):
        keys = ["epoch", "train_loss"] if keys is None else keys
        assert isinstance(keys, list), "Keys must be a list."
        for key in keys:
            assert key in self.history, "Key not in history."
            print(key, ": ", self.history[key][-1])

    def visualize_and_store_history(self):
        """on request (settings.save_history) the weights and `training_history.json`; on request (show_fig / save_fig) one figure of
        the two losses over the epochs - matplotlib is imported only then"""
        st, res = self.settings, self._results()
        if st.save_history:
            self.approx_mpc.save_to_state_dict(res / "approx_mpc.pth")
            (res / "training_history.json").write_text(json.dumps(self.history, indent=4))
        if st.show_fig or st.save_fig:
            plt = _pyplot()
            fig, ax = plt.subplots()
            for key in ("train_loss", "val_loss"):
                ax.semilogy(self.history["epoch"], self.history[key], label=key)
            ax.set_xlabel("epoch")
            ax.legend()
            if st.save_fig:
                fig.savefig(res / "training_history.png")
            if st.show_fig:
                plt.show()
            plt.close(fig)

    def _loss(self, x, y, js=None):
        """mse(net(x), y), plus sobolev_weight mse(J_net(x), js) over the rows of js that are all finite when the weight is positive"""
        w = self.settings.sobolev_weight
        if not w > 0:
            return torch.nn.functional.mse_loss(self.approx_mpc(x), y)
        out, J = network_jacobian(self.approx_mpc.net, x)
        loss_u = torch.nn.functional.mse_loss(out, y)
        labelled = torch.isfinite(js).all(dim=2).all(dim=1)
        loss_j = torch.nn.functional.mse_loss(J[labelled], js[labelled]) if bool(labelled.any()) else torch.zeros((), dtype=loss_u.dtype, device=loss_u.device)
        self._terms.append((loss_u.item(), loss_j.item()))
        return loss_u + w * loss_j

    def train_step(self, optim, x, y, js=None):
        """one optimiser step on one mini-batch -> its loss"""
        loss = self._loss(x, y, js)
        optim.zero_grad()
        loss.backward()
        optim.step()
        return loss.item()

    def train_epoch(self, optim, train_loader):
        """mean loss over the mini-batches of one pass"""
        return fmean(self.train_step(optim, *batch) for batch in train_loader)

    def validation_step(self, x, y, js=None):
        with torch.no_grad():
            return self._loss(x, y, js).item()

    def validation_epoch(self, val_loader):
        return fmean(self.validation_step(*batch) for batch in val_loader)

    def _mean_terms(self, prefix):
        """the two terms of the loss, averaged over the mini-batches since the last call (Sobolev training only)"""
        terms, self._terms = self._terms, []
        return {prefix + "_u": fmean(t[0] for t in terms), prefix + "_j": fmean(t[1] for t in terms)} if terms else {}

    def sensitivity_error(self, data=None) -> dict:
        """The network's Jacobian against the stored MPC sensitivities, in the network's coordinates, over the rows of the `_opt` file
        (or of `data`, a table with the same columns) whose labels are all finite -> {"mse", "max_abs", "n_rows", "n_labelled"}.  The
        Jacobian comes from ApproxMPC.jacobian_batch when a device is there, otherwise from the torch recursion."""
        assert self.flags["setup"] == True, "MPC was not setup yet. Please call Trainer.setup()."      # noqa: E712
        st, a = self.settings, self.approx_mpc
        source = Path(st.data_dir).joinpath(st.dataset_name).joinpath("data_" + st.dataset_name + "_opt.pkl")
        if data is None:
            with open(source, "rb") as f:
                data = pkl.load(f)
        xs, _, Js = self._scaled_columns(data, True, source)
        labelled = torch.isfinite(Js).all(dim=2).all(dim=1)
        out = {"n_rows": int(Js.shape[0]), "n_labelled": int(labelled.sum())}
        if not out["n_labelled"]:
            return {**out, "mse": float("nan"), "max_abs": float("nan")}
        Js = Js[labelled].double()
        if torch.cuda.is_available():
            m = a.mpc.model
            rows = labelled.numpy()
            stack = lambda key, n: np.stack([np.asarray(v, dtype=float).reshape(-1) for v in data[key]]).reshape(-1, n)[rows]      # noqa: E731
            r = a.jacobian_batch(stack("x0", m.n_x), stack("u_prev", m.n_u) if a.rterm else None, clip_to_bounds=False)
            J = torch.from_numpy(np.concatenate((r["du_dx"], r["du_du_prev"]), axis=2) if a.rterm else r["du_dx"])
            if a.settings.scaling:
                J = J * a.x_range.reshape(1, 1, -1) / a.y_range.reshape(1, -1, 1)
        else:
            with torch.no_grad():
                J = network_jacobian(a.net, xs[labelled].to(self.device))[1].double().cpu()
        err = J - Js
        return {**out, "mse": float(err.square().mean()), "max_abs": float(err.abs().max())}

    def default_training(self):
        assert self.flags["setup"] == True, "MPC was not setup yet. Please call Trainer.setup()."      # noqa: E712
        st = self.settings
        train_loader, val_loader, optimizer = self.load_data()
        for epoch in range(st.n_epochs):
            self._terms = []
            row = {"epoch": epoch, "train_loss": self.train_epoch(optimizer, train_loader), "lr": optimizer.param_groups[0]["lr"]}
            row.update(self._mean_terms("train_loss"))
            row["val_loss"] = self.validation_epoch(val_loader)
            row.update(self._mean_terms("val_loss"))
            for key, val in row.items():
                self.log_value(val, key)
            if (epoch + 1) % st.print_frequency == 0:
                self.print_last_entry(keys=["epoch", "train_loss", "val_loss"])
                print("-" * 31)
            if st.scheduler_flag:
                self.lr_scheduler.step(row["val_loss"])
                if optimizer.param_groups[0]["lr"] < self.scheduler_settings.min_lr:
                    break
        self.approx_mpc._epoch += 1                                      # the next step packs the trained weights
        self.approx_mpc.save_to_state_dict(self._results() / "approx_mpc.pth")
        if st.show_fig or st.save_fig or st.save_history:
            self.visualize_and_store_history()
