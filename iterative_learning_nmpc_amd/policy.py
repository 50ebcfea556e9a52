"""Host mirror of the reference's policy network and behaviour-cloning step on the device.

    GoalConditionedPolicyNet(input_size, output_size, num_hidden_layer, hidden_dim, batch_norm)
        DAgger/utils/network.py:7-81          -> DevicePolicy (forward = eval mode)
    BehavioralCloning.train_network, inner loop   DAgger/utils/train_locosafedagger.py:93-102
        -> DevicePolicy.train_step(x, y, lr)   (L1 loss, Adam)
    one epoch of that loop over a weighted loader   train_locosafedagger.py:93-102
        -> DevicePolicy.train_epoch(db, batch_size, n_batches, lr, seed)
    the validation loss of an epoch                 train_locosafedagger.py:129-132
        -> DevicePolicy.loss(x, y)

The kernels are in csrc/nmpc_policy.hip behind include/nmpc_policy.h; tensors stay on the device
(torch is the container only).  There is no CPU path."""
import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream


def parameter_layout(n_in, n_out, n_hidden, hidden, batch_norm):
    """[(name, shape, offset)] of the flat parameter vector (the order of net.parameters())."""
    items, off = [], 0
    for l in range(n_hidden):
        fan_in = n_in if l == 0 else hidden
        names = [(f"net.{l}.W", (hidden, fan_in)), (f"net.{l}.b", (hidden,))]
        if batch_norm:
            names += [(f"net.{l}.gamma", (hidden,)), (f"net.{l}.beta", (hidden,))]
        for name, shape in names:
            items.append((name, shape, off)); off += int(np.prod(shape))
    for name, shape in ((f"net.{n_hidden}.W", (n_out, hidden)), (f"net.{n_hidden}.b", (n_out,))):
        items.append((name, shape, off)); off += int(np.prod(shape))
    return items, off


class DevicePolicy:
    """The reference's MLP policy with its parameters, BatchNorm buffers and Adam state on one GPU."""

    def __init__(self, input_size: int, output_size: int, num_hidden_layer: int = 3, hidden_dim: int = 512,
                 batch_norm: bool = True, batch_max: int = 1024, device="cuda:0", seed: Optional[int] = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("DevicePolicy needs a HIP device; there is no CPU path")
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.dims = (int(input_size), int(output_size), int(num_hidden_layer), int(hidden_dim), bool(batch_norm))
        self.batch_max = int(batch_max)
        d = _lib.NmpcPolicyDims(*self.dims[:4], int(batch_norm), self.batch_max)
        self._h = ctypes.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self.lib.nmpc_policy_create(ctypes.byref(d), idx, ctypes.byref(self._h)), None, "nmpc_policy_create", "policy")
        self.items, self.n_theta = parameter_layout(*self.dims)
        assert self.n_theta == self.lib.nmpc_policy_param_count(self._h)
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._input_noise = None        # set_input_noise: the attached sigma
        if seed is not None:
            self.init_weight(seed)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self.lib.nmpc_policy_destroy(h)
            self._h = None

    # -- parameters ---------------------------------------------------------------------------------
    def init_weight(self, seed: int = 0):
        """Kaiming-normal weights (fan_in, relu), zero biases, gamma = 1, beta = 0 (network.py:59-70)."""
        n_in, n_out, L, hidden, bn = self.dims
        g = torch.Generator().manual_seed(seed)
        theta = torch.zeros(self.n_theta)
        for name, shape, off in self.items:
            n = int(np.prod(shape))
            if name.endswith(".W"):
                theta[off:off + n] = (torch.randn(shape, generator=g) * (2.0 / shape[1]) ** 0.5).reshape(-1)
            elif name.endswith(".gamma"):
                theta[off:off + n] = 1.0
        self.set_parameters(theta, torch.zeros(L, hidden), torch.ones(L, hidden))

    def _staged(self, t, numel: int, what: str) -> torch.Tensor:
        """`t` as contiguous fp32 on the policy's device, its length checked before anything is copied there"""
        t = torch.as_tensor(t, dtype=torch.float32)
        if t.numel() != numel:
            raise ValueError(f"{what} needs {numel} elements, got {t.numel()}")
        return t.contiguous().to(self.device)

    def _set(self, name: str, *args):
        """a set call of the library on staged tensors, which go out of scope afterwards: the stream is waited for"""
        _lib.check(getattr(self.lib, name)(self._h, *args, stream(self.device)), self._h, name, "policy")
        torch.cuda.current_stream(self.device).synchronize()

    def set_parameters(self, theta, running_mean=None, running_var=None):
        n_in, n_out, L, hidden, bn = self.dims
        theta = self._staged(theta, self.n_theta, "theta")
        rm = self._staged(running_mean, L * hidden, "running_mean") if bn else None
        rv = self._staged(running_var, L * hidden, "running_var") if bn else None
        self._set("nmpc_policy_set_params", ptr(theta), ptr(rm), ptr(rv))

    def get_parameters(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        n_in, n_out, L, hidden, bn = self.dims
        theta = torch.empty(self.n_theta, dtype=torch.float32, device=self.device)
        # (without BatchNorm there are no running statistics: the library leaves these two as they are -- zeros / ones,
        #  the state of a fresh BatchNorm layer, rather than uninitialised memory)
        rm = torch.zeros(L, hidden, dtype=torch.float32, device=self.device)
        rv = torch.ones(L, hidden, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nmpc_policy_get_params(self._h, ptr(theta), ptr(rm), ptr(rv), stream(self.device)),
                   self._h, "nmpc_policy_get_params", "policy")
        return theta, rm, rv

    def get_optimizer_state(self) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """Adam's moments (m, v: fp32 [n_theta] on the device, in the layout of theta) and the count of steps taken."""
        m = torch.empty(self.n_theta, dtype=torch.float32, device=self.device)
        v = torch.empty(self.n_theta, dtype=torch.float32, device=self.device)
        step = ctypes.c_longlong()
        _lib.check(self.lib.nmpc_policy_get_opt_state(self._h, ptr(m), ptr(v), ctypes.byref(step), stream(self.device)),
                   self._h, "nmpc_policy_get_opt_state", "policy")
        return m, v, int(step.value)

    def set_optimizer_state(self, m, v, step: int):
        """Resume from a checkpoint: after `set_parameters` (which resets the optimiser), put back what
        `get_optimizer_state` gave."""
        m, v = self._staged(m, self.n_theta, "m"), self._staged(v, self.n_theta, "v")
        self._set("nmpc_policy_set_opt_state", ptr(m), ptr(v), int(step))

    def load_state_dict(self, state: Dict[str, "np.ndarray"]):
        """Parameters from the reference's state_dict ('net.<i>.weight', BatchNorm buffers ...)."""
        n_in, n_out, L, hidden, bn = self.dims
        theta = np.zeros(self.n_theta, np.float32)
        view = {n: theta[o:o + int(np.prod(s))].reshape(s) for n, s, o in self.items}
        rm, rv = np.zeros((L, hidden), np.float32), np.ones((L, hidden), np.float32)
        idx = 0
        for l in range(L + 1):
            view[f"net.{l}.W"][:] = np.asarray(state[f"net.{idx}.weight"]); view[f"net.{l}.b"][:] = np.asarray(state[f"net.{idx}.bias"])
            idx += 1
            if l < L:
                if bn:
                    view[f"net.{l}.gamma"][:] = np.asarray(state[f"net.{idx}.weight"]); view[f"net.{l}.beta"][:] = np.asarray(state[f"net.{idx}.bias"])
                    rm[l] = np.asarray(state[f"net.{idx}.running_mean"]); rv[l] = np.asarray(state[f"net.{idx}.running_var"])
                    idx += 1
                idx += 1                                  # ReLU
        self.set_parameters(theta, rm, rv)

    # -- forward / training ---------------------------------------------------------------------------
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """network.eval(); network(x)"""
        B = x.shape[0]
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape == (B, self.dims[0])
        y = torch.empty(B, self.dims[1], dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nmpc_policy_forward(self._h, B, ptr(x), ptr(y), stream(self.device)), self._h,
                   "nmpc_policy_forward", "policy")
        return y

    __call__ = forward

    def train_step(self, x: torch.Tensor, y: torch.Tensor, lr: float = 1e-3, return_pred: bool = False):
        """optimizer.zero_grad(); loss = L1Loss(network(x), y); loss.backward(); optimizer.step().
        Returns the loss as a device scalar (and the train-mode prediction)."""
        B = x.shape[0]
        assert x.is_cuda and y.is_cuda and x.dtype == y.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous()
        assert x.shape == (B, self.dims[0]) and y.shape == (B, self.dims[1])
        pred = torch.empty(B, self.dims[1], dtype=torch.float32, device=self.device) if return_pred else None
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nmpc_policy_train_step(self._h, B, ptr(x), ptr(y), float(lr), ptr(loss), ptr(pred),
                                                   stream(self.device)), self._h, "nmpc_policy_train_step", "policy")
        return (loss, pred) if return_pred else loss

    def train_epoch(self, db, batch_size: int, n_batches: int, lr: float, seed: int, weights: Optional[torch.Tensor] = None,
                    return_idx: bool = False):
        """`n_batches` training steps in one library call (train_locosafedagger.py:93-102 over a WeightedRandomSampler
        loader): step t trains on `db.batch(idx[t])` with idx = weighted_sample(weights, n_batches * batch_size,
        seed).reshape(n_batches, batch_size), bit for bit, but the prefix sums of the weights are made once, and index,
        batch and staging tensors never surface.  db: a `DeviceDatabase` (its goal type and normalisation switch as in
        `db.batch`); weights: fp32 [len(db)] on the device, default `db.weights[:len(db)]`; a row of weight zero is never
        drawn.  Returns the losses before each step as a device vector [n_batches] (and idx [n_batches, batch_size],
        int32)."""
        src = db.batch_source()
        n = len(db)
        w = db.weights[:n] if weights is None else weights
        assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.shape == (n,)
        scratch = torch.empty(self.lib.nmpc_policy_train_epoch_scratch(n), dtype=torch.float64, device=self.device)
        losses = torch.empty(n_batches, dtype=torch.float32, device=self.device)
        idx = torch.empty(n_batches, batch_size, dtype=torch.int32, device=self.device) if return_idx else None
        _lib.check(self.lib.nmpc_policy_train_epoch(self._h, ctypes.byref(src), ptr(w), int(batch_size), int(n_batches),
                                                    int(seed) & (2 ** 64 - 1), float(lr), ptr(scratch), ptr(losses), ptr(idx),
                                                    stream(self.device)), self._h, "nmpc_policy_train_epoch", "policy")
        return (losses, idx) if return_idx else losses

    def set_input_noise(self, sigma=None, seed: int = 0, epoch0: int = 0):
        """nmpc_policy_set_input_noise: noise on the input columns of the batches `train_epoch` trains on, so that a policy
        deployed behind noisy sensors (`BatchedTorqueLayer.set_noise`) is trained on inputs like the ones it will see.  sigma: a
        float array or tensor [n], 1 <= n <= n_in, finite and not negative, in the units of the RAW input columns 0 .. n-1
        (`torque.training_sigma` makes one of a sensor table).  While attached every `train_epoch` adds sigma[j] g to column j of
        each staged batch by one more launch per batch -- divided by the column's states_std where the database normalises it --
        g the variate of the sensor rule at counter (t * batch_size + i, epoch, j, 1) for row i of batch t, and then moves the
        policy's noise epoch (`input_noise_epoch`) on by one; a column with sigma 0 is not written.  `train_step`, `forward` and
        `loss` never draw: validation stays on clean rows.  seed: 64 bits; epoch0: the epoch of the next `train_epoch`.
        Host input is validated (ValueError) and uploaded; the policy keeps the vector alive while it is attached.
        `set_input_noise(None)` detaches; detached, every call makes the launches and gives the bits it gives without."""
        if sigma is None:
            self._input_noise = None
            _lib.check(self.lib.nmpc_policy_set_input_noise(self._h, None, 0, 0, 0), self._h, "nmpc_policy_set_input_noise", "policy")
            return
        try:
            host = sigma.detach().cpu().numpy() if isinstance(sigma, torch.Tensor) else sigma
            host = np.asarray(host, dtype=np.float32)
        except (TypeError, ValueError) as e:
            raise ValueError("input noise: sigma: need a float array [n]") from e
        if host.ndim != 1 or not 1 <= host.shape[0] <= self.dims[0]:
            raise ValueError(f"input noise: sigma: expected [n] with 1 <= n <= {self.dims[0]}, got {tuple(host.shape)}")
        if not np.isfinite(host).all():
            raise ValueError("input noise: sigma must be finite")
        if not (host >= 0.0).all():
            raise ValueError("input noise: sigma must not be negative")
        epoch0 = int(epoch0)
        if not 0 <= epoch0 < 2 ** 63:
            raise ValueError("input noise: epoch0 must be in [0, 2^63)")
        key = int(seed) & (2 ** 64 - 1)                   # the 64 bits of the key, as the signed argument that carries them
        dev = torch.tensor(host, device=self.device)
        _lib.check(self.lib.nmpc_policy_set_input_noise(self._h, ptr(dev), dev.shape[0], key - 2 ** 64 if key >= 2 ** 63 else key, epoch0),
                   self._h, "nmpc_policy_set_input_noise", "policy")
        self._input_noise = dev

    @property
    def input_noise_epoch(self) -> Optional[int]:
        """nmpc_policy_input_noise_epoch: the epoch the next `train_epoch` draws its input noise at, or None with nothing attached"""
        if self._input_noise is None:
            return None
        epoch = ctypes.c_longlong()
        _lib.check(self.lib.nmpc_policy_input_noise_epoch(self._h, ctypes.byref(epoch)), self._h, "nmpc_policy_input_noise_epoch", "policy")
        return epoch.value

    def input_noise(self, X: torch.Tensor, epoch: int, first_sample: int = 0, s_std=None, s_first: int = 1) -> torch.Tensor:
        """nmpc_policy_input_noise_batch: the attached input noise on the first n columns of X, a float32 [B, >= n] tensor on the
        policy's device with dense rows (a slice [:, :k] of a wider contiguous tensor is taken with its stride), IN PLACE, row i
        as sample first_sample + i of `epoch`; the policy's own epoch is neither read nor moved.  s_std: float64 [>= n], the
        statistics X was normalised with from column s_first on (None: X is raw).  What `train_epoch` does to batch t with
        first_sample = t * batch_size while the vector is attached.  -> X."""
        if not isinstance(X, torch.Tensor) or X.dtype != torch.float32 or X.dim() != 2 or X.device != self.device \
                or (X.shape[0] > 0 and X.stride(1) != 1) or (X.shape[0] > 1 and X.stride(0) < X.shape[1]):
            raise ValueError(f"X: need a float32 [B, columns] tensor with dense rows on {self.device}")
        n = 0 if self._input_noise is None else self._input_noise.shape[0]
        if X.shape[1] < n:
            raise ValueError(f"X: need at least the {n} columns of the attached sigma, got {X.shape[1]}")
        if s_std is not None:
            s_std = torch.as_tensor(s_std, dtype=torch.float64, device=self.device).contiguous()
            if s_std.dim() != 1 or s_std.shape[0] < n:
                raise ValueError(f"s_std: expected [>= {n}]")
        epoch, first_sample = int(epoch), int(first_sample)
        if not (0 <= epoch < 2 ** 63 and 0 <= first_sample < 2 ** 63):
            raise ValueError("input noise: epoch and first_sample must be in [0, 2^63)")
        x_stride = X.stride(0) if X.shape[0] > 1 else X.shape[1]
        _lib.check(self.lib.nmpc_policy_input_noise_batch(self._h, X.shape[0], ptr(X), x_stride, ptr(s_std), int(s_first), epoch,
                                                          first_sample, stream(self.device)),
                   self._h, "nmpc_policy_input_noise_batch", "policy")
        return X

    def loss(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """network.eval(); L1Loss(network(x), y) as a device scalar, for any number of rows (the validation loss of
        train_locosafedagger.py:129-132); nothing of the policy changes."""
        n = x.shape[0]
        assert x.is_cuda and y.is_cuda and x.dtype == y.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous()
        assert x.shape == (n, self.dims[0]) and y.shape == (n, self.dims[1])
        out = torch.empty(1, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nmpc_policy_loss(self._h, n, ptr(x), ptr(y), ptr(out), stream(self.device)), self._h,
                   "nmpc_policy_loss", "policy")
        return out


def weighted_sample(weights: torch.Tensor, num_samples: int, seed: int) -> torch.Tensor:
    """WeightedRandomSampler(weights, num_samples, replacement=True) on device weights
    (test_train_policy.py:128-134): int32 indices [num_samples], reproducible for a seed."""
    lib = _lib.load()
    w = weights.reshape(-1)
    assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()
    n = w.numel()
    scratch = torch.empty(n + n // 2048 + 2, dtype=torch.float64, device=w.device)
    idx = torch.empty(num_samples, dtype=torch.int32, device=w.device)
    _lib.check(lib.nmpc_weighted_sample(ptr(w), n, int(num_samples), int(seed) & (2 ** 64 - 1), ptr(scratch), ptr(idx),
                                        stream(w.device)), None, "nmpc_weighted_sample", "policy")
    return idx


def gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """Batch assembly behind the sampler: src[idx] for a [rows, features] fp32 table."""
    lib = _lib.load()
    assert src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 2
    assert idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous()
    dst = torch.empty(idx.numel(), src.shape[1], dtype=torch.float32, device=src.device)
    _lib.check(lib.nmpc_gather_rows(ptr(src), src.shape[0], src.shape[1], ptr(idx), idx.numel(), ptr(dst), stream(src.device)),
               None, "nmpc_gather_rows", "policy")
    return dst
