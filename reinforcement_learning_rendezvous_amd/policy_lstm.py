"""
The recurrent policy of the reference's main_rnn.py (sb3-contrib ``RecurrentPPO("MlpLstmPolicy")``, also tune_policy.py:80,
tune_algorithm.py:68): ``RecurrentActorCriticPolicy`` with ONE LSTM layer of ``lstm_hidden_size`` units in front of the
``mlp_extractor`` trunk, and separate LSTMs for actor and critic (``shared_lstm=False``, ``enable_critic_lstm=True``, the defaults).
Per env row::

    h, c   <- (1 - episode_start) * (h, c)
    h', c' =  LSTMCell(obs, (h, c))                     torch.nn.LSTM(17, H), gate order i, f, g, o
    actor:  mean = action_net(policy_net(h'));   critic: value = value_net(value_net_trunk(h')) from its OWN LSTM

On the GPU a step is two hand-written HIP kernels per network (csrc/rdv_policy_lstm.h, through the C ABI: rdv_lstm_act /
rdv_lstm_value); the state lives in device memory, owned by the handle.  ``backend="torch"`` (and CPU observations) run the plain
``torch.nn.LSTM`` and ``Linear`` modules with the same semantics, which the tests use as the kernels' reference.  Served: H in
{32, 64, 128, 256}, trunks of 1..4 hidden layers of 16 / 32 / 64 with tanh / ReLU / sigmoid.  More LSTM layers, a shared LSTM, a critic
without an LSTM and any other H raise ValueError.

``LstmPolicySet`` holds P such policies of one architecture over one batch, member g owning a range of rows: one cell launch and one
trunk launch per call for all members (include/rdv.h, "Recurrent policy sets"), the state of all rows owned by the set.
"""
import ctypes as C
import io
import json
import zipfile

import numpy as np
import torch

from .policy import ACTIVATIONS, _HipHandles, _Members, _ptrs, _trunk_keys, infer_arch, parse_activation, parse_net_arch

LSTM_HIDDEN_SIZES = (32, 64, 128, 256)
_LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def check_lstm_config(lstm_hidden_size, n_lstm_layers=1, shared_lstm=False, enable_critic_lstm=True):
    """The refusals of include/rdv.h ("The recurrent policy"), by name, on the host."""
    if int(n_lstm_layers) != 1:
        raise ValueError(f"n_lstm_layers = {n_lstm_layers}: one LSTM layer is served")
    if shared_lstm:
        raise ValueError("shared_lstm = True: separate actor and critic LSTMs are served (the main_rnn.py defaults)")
    if not enable_critic_lstm:
        raise ValueError("enable_critic_lstm = False: a critic without an LSTM of its own is not served")
    if int(lstm_hidden_size) not in LSTM_HIDDEN_SIZES:
        raise ValueError(f"lstm_hidden_size = {lstm_hidden_size} is not one of {LSTM_HIDDEN_SIZES}")


class _LstmRows(_HipHandles):
    """What LstmPolicy and LstmPolicySet share: the rows whose state (h, c) a recurrent handle owns, the pending episode-start flags and their
    mirror, and the act / value / advantages calls on the handles of ``_create_handle``.  The class gives ``lstm_hidden_size``, ``n_rows``,
    ``backend``, ``noise_seed``, ``noise_env_offset``, ``_calls``, ``_state``, ``_pending``, ``_dev_pending``, and for the PyTorch path ``_module_device``,
    ``_forward_torch(prefix, obs, start, commit)`` (one step of the modules: means [n, 6] or values [n, 1]) and
    ``_sample_torch(mean, deterministic, generator, log_prob_out)`` (the unclipped action; ``log_prob_out`` [n] or None is filled)."""

    def _rows(self, n):
        if self.n_rows is None:
            self.n_rows = int(n)
        if int(n) != self.n_rows:
            raise ValueError(f"{n} rows, the policy owns the state of {self.n_rows}")
        return self.n_rows

    def _torch_state(self, prefix, device):
        if self.n_rows is None:
            raise ValueError("the number of rows is not known yet: pass n_rows or evaluate the policy once")
        st = self._state.get(prefix)
        if st is None:
            st = [torch.zeros((self.n_rows, self.lstm_hidden_size), dtype=torch.float32, device=device) for _ in range(2)]
        elif st[0].device != device:
            st = [t.to(device) for t in st]
        self._state[prefix] = st
        return st

    def _device_flags(self, prefix, device):
        """The mirror of a HIP handle's pending flags ON THE DEVICE: ONE uint8 [rows] tensor per prefix and device, allocated when the
        handle is created (outside any stream capture) and only ever written in place.  Work recorded into a HIP graph therefore reads
        the flags that the replay or the eager call before it left, not the tensor of the recording.  None: no handle on ``device``."""
        device = torch.device(device)
        if device.type != "cuda":
            return None
        return self._dev_pending.get((prefix, device.index if device.index is not None else torch.cuda.current_device()))

    def _pending_flags(self, prefix, device):
        """The pending episode-start flags as a uint8 [rows] tensor: the handle's mirror on ``device`` itself where there is one."""
        flags = self._device_flags(prefix, device)
        if flags is not None:
            return flags
        p = self._pending[prefix]
        if isinstance(p, torch.Tensor):
            return p.to(device)
        return torch.full((self.n_rows,), 1 if p else 0, dtype=torch.uint8, device=device)

    def _set_pending(self, prefix, value, device=None):
        """What a call leaves pending: True (every row), False (none) or a uint8 [rows] tensor (``done[T-1]`` of a rollout).  Written in
        place into the mirror of the handle on ``device``; the host value ``_pending[prefix]`` is the PyTorch path's, and that of the time
        before a handle exists."""
        flags = None if device is None else self._device_flags(prefix, device)
        if flags is None:
            self._pending[prefix] = value.clone() if isinstance(value, torch.Tensor) else value
        elif isinstance(value, torch.Tensor):
            flags.copy_(value)
        else:
            flags.fill_(1 if value else 0)

    def state_at_start(self, prefix="l", device=None):
        """``(h, c)`` as the next rollout's first step will see it: the state, zero where an episode start is pending — what
        RecurrentPPO's buffer keeps for a sequence start (``RendezvousBatch.rollout`` returns it as ``lstm_state0``)."""
        h, c = self._get_state(prefix, device)
        keep = (self._pending_flags(prefix, h.device) == 0).to(h.dtype)[:, None]
        return h * keep, c * keep

    def _use_hip(self, obs):
        return self.backend == "hip" or (self.backend == "auto" and obs.is_cuda and obs.dtype == torch.float32)

    def _handle(self, prefix, device):
        if self.n_rows is None:
            raise ValueError("the number of rows is not known yet: pass n_rows or evaluate the policy once")
        h = super()._handle(prefix, device)
        device = torch.device(device)
        key = (prefix, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._dev_pending:          # with the handle: the mirror of its flags starts from the host value (every row, as created)
            self._dev_pending[key] = self._pending_flags(prefix, torch.device("cuda", key[1])).clone()
        return h

    def close(self):
        super().close()
        self._dev_pending = {}

    def _get_state(self, prefix, device=None):
        table = self._hip if prefix == "l" else self._hip_critic
        if self.backend != "torch" and table:
            from . import _native as N
            idx = next(iter(table)) if device is None or torch.device(device).index is None else torch.device(device).index
            dev = torch.device("cuda", idx)
            h = torch.empty((self.n_rows, self.lstm_hidden_size), dtype=torch.float32, device=dev)
            c = torch.empty_like(h)
            N.check(N.lib().rdv_lstm_get_state(table[idx], C.c_void_p(h.data_ptr()), C.c_void_p(c.data_ptr()), self._stream(dev)))
            return h, c
        st = self._torch_state(prefix, torch.device(device) if device is not None else self._module_device)
        return st[0].clone(), st[1].clone()

    def _set_state(self, prefix, hc, device=None):
        h, c = hc
        if self.backend != "torch" and isinstance(h, torch.Tensor) and h.is_cuda:
            from . import _native as N
            self._rows(h.shape[0])
            h, c = h.to(torch.float32).contiguous(), c.to(torch.float32).contiguous()
            N.check(N.lib().rdv_lstm_set_state(self._handle(prefix, h.device), C.c_void_p(h.data_ptr()), C.c_void_p(c.data_ptr()), self._stream(h.device)))
            self._set_pending(prefix, False, h.device)
            return
        h = torch.as_tensor(h, dtype=torch.float32)
        c = torch.as_tensor(c, dtype=torch.float32)
        self._rows(h.shape[0])
        st = self._torch_state(prefix, h.device)
        st[0].copy_(h); st[1].copy_(c)
        self._pending[prefix] = False

    @property
    def state(self):
        """The actor's ``(h, c)``, [rows, H] float32 each, plain row-major (a copy)."""
        return self._get_state("l")

    @state.setter
    def state(self, hc):
        self._set_state("l", hc)

    @property
    def critic_state(self):
        return self._get_state("v")

    @critic_state.setter
    def critic_state(self, hc):
        self._set_state("v", hc)

    @torch.no_grad()
    def reset_state(self, mask=None):
        """Zero state for the rows of ``mask`` (None: every row), actor and critic alike."""
        from . import _native as N
        for prefix, table in (("l", self._hip), ("v", self._hip_critic)):
            for idx, hnd in table.items():
                dev = torch.device("cuda", idx)
                m = None if mask is None else torch.as_tensor(mask).to(dev, torch.uint8).contiguous()
                N.check(N.lib().rdv_lstm_reset_state(hnd, None if m is None else C.c_void_p(m.data_ptr()), self._stream(dev)))
            st = self._state.get(prefix)
            if st is not None:
                keep = torch.zeros(self.n_rows, dtype=torch.bool, device=st[0].device) if mask is None else \
                    ~torch.as_tensor(mask).to(st[0].device).bool()
                st[0].mul_(keep[:, None]); st[1].mul_(keep[:, None])

    @staticmethod
    def _aligned(obs):
        """Contiguous rows at a 16-byte aligned address, as the kernels read them (row t of a [T, N, 17] tensor is not when N % 4 != 0)."""
        obs = obs.contiguous()
        return obs.clone() if obs.data_ptr() % 16 else obs

    @staticmethod
    def _flags(episode_start, n, device):
        if episode_start is None:
            return None
        f = torch.as_tensor(np.asarray(episode_start) if not isinstance(episode_start, torch.Tensor) else episode_start)
        if f.shape != (n,):
            raise ValueError(f"episode_start: expected {n} flags, got {tuple(f.shape)}")
        return (f != 0).to(device, torch.uint8).contiguous()

    @torch.no_grad()
    def act(self, obs, episode_start=None, deterministic=True, generator=None, out=None, env_id_offset=None, raw_out=None, log_prob_out=None):
        """One step of the actor on observations [n, 17], n the policy's rows: the clipped action; the state advances.
        ``episode_start``: [n] flags (None: no row starts an episode).  HIP backend: noise keyed by (noise_seed, env_id_offset + i,
        call counter), as ``MlpPolicy.act``; ``raw_out`` [n, 6] / ``log_prob_out`` [n] receive the unclipped sample and its log-density.
        Inside a stream capture (a HIP graph) pass ``episode_start`` as a device tensor made before the recording: a NumPy array or a
        CPU tensor becomes a host-to-device copy, which does not belong in a capture."""
        n = self._rows(obs.shape[0])
        if self._use_hip(obs):
            from . import _native as N
            if generator is not None:
                self.noise_seed = int(generator.initial_seed())
            offset = self.noise_env_offset if env_id_offset is None else int(env_id_offset)
            obs = self._aligned(obs)
            flags = self._flags(episode_start, n, obs.device)
            if out is None:
                out = torch.empty((n, 6), dtype=torch.float32, device=obs.device)
            ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
            N.check(N.lib().rdv_lstm_act(self._handle("l", obs.device), ptr(obs), ptr(flags), ptr(out), ptr(raw_out), ptr(log_prob_out), n,
                                         int(bool(deterministic)), C.c_uint64(self.noise_seed), C.c_uint64(self._calls), C.c_uint64(offset),
                                         self._stream(obs.device)))
            self._calls += 1
            self._set_pending("l", False, obs.device)
            return out
        mean = self._forward_torch("l", obs, self._flags(episode_start, n, obs.device))
        a = self._sample_torch(mean, deterministic, generator, log_prob_out)
        if raw_out is not None:
            raw_out.copy_(a)
        res = torch.clamp(a, -1.0, 1.0)
        if out is not None:
            out.copy_(res)
            return out
        return res

    @torch.no_grad()
    def value(self, obs, episode_start=None, commit=True, out=None):
        """One step of the critic on observations [n, 17]: values [n].  ``commit=False`` evaluates without writing the critic's state
        (sb3-contrib's ``predict_values`` for the value of the last observation).  Inside a stream capture ``episode_start`` is a device
        tensor made before the recording, as for ``act``."""
        n = self._rows(obs.shape[0])
        if self._use_hip(obs):
            from . import _native as N
            obs = self._aligned(obs)
            flags = self._flags(episode_start, n, obs.device)
            if out is None:
                out = torch.empty((n,), dtype=torch.float32, device=obs.device)
            N.check(N.lib().rdv_lstm_value(self._handle("v", obs.device), C.c_void_p(obs.data_ptr()), None if flags is None else C.c_void_p(flags.data_ptr()),
                                           C.c_void_p(out.data_ptr()), n, int(bool(commit)), self._stream(obs.device)))
            if commit:
                self._set_pending("v", False, obs.device)
            return out
        v = self._forward_torch("v", obs, self._flags(episode_start, n, obs.device), commit=commit)[:, 0]
        if out is not None:
            out.copy_(v)
            return out
        return v

    @torch.no_grad()
    def advantages(self, ro, gamma=0.99, gae_lambda=0.95, out=None):
        """``MlpPolicy.advantages`` for the recurrent critic: T committing critic steps in time order over ``ro["obs"]`` (episode starts:
        the critic's pending flags, then ``ro["done"][t-1]``), one non-committing step on ``ro["last_obs"]`` with ``done[T-1]``, GAE.
        Also records ``ro["lstm_critic_state0"]``, the critic's ``(h, c)`` as step 0 sees it (``state_at_start("v")``), as ``rollout``
        records the actor's ``lstm_state0``: ``ppo_sequence_grad`` starts from both."""
        from . import advantages as A
        obs = ro["obs"]
        if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[2] != 17:
            raise ValueError(f"obs: expected a [T,N,17] tensor, got {tuple(getattr(obs, 'shape', ()))}")
        T, n, dev = int(obs.shape[0]), int(obs.shape[1]), obs.device
        self._rows(n)
        A.check_tensor(obs, "obs", (T, n, 17), torch.float32, dev)
        A.check_tensor(ro["reward"], "reward", (T, n), torch.float32, dev)
        A.check_tensor(ro["done"], "done", (T, n), torch.uint8, dev)
        A.check_tensor(ro["last_obs"], "last_obs", (n, 17), torch.float32, dev)
        A.check_discounts(gamma, gae_lambda)
        if self.backend != "torch" and obs.is_cuda:
            self._handle("v", dev)
        ro["lstm_critic_state0"] = self.state_at_start("v", dev)
        src = out if out is not None else ro
        for name, shape in dict(values=(T, n), last_value=(n,), advantages=(T, n), returns=(T, n)).items():
            t = src.get(name)
            if t is None or tuple(t.shape) != shape or t.device != dev:
                t = torch.empty(shape, dtype=torch.float32, device=dev)
            ro[name] = t
        if self.backend != "torch" and obs.is_cuda:
            from . import _native as N
            rows = N.RolloutOut(obs.data_ptr(), None, ro["reward"].data_ptr(), ro["done"].data_ptr(), None, ro["last_obs"].data_ptr())
            ao = N.AdvantageOut(*[ro[f].data_ptr() for f, _ in N.AdvantageOut._fields_])
            N.check(N.lib().rdv_rollout_advantages(self._handle("v", dev), C.byref(rows), T, n, float(gamma), float(gae_lambda), C.byref(ao),
                                                   self._stream(dev)))
            self._set_pending("v", ro["done"][T - 1], dev)
            return ro
        for t in range(T):
            flags = self._pending_flags("v", dev) if t == 0 else ro["done"][t - 1]
            self.value(obs[t], episode_start=flags, out=ro["values"][t])
        self.value(ro["last_obs"], episode_start=ro["done"][T - 1], commit=False, out=ro["last_value"])
        self._pending["v"] = ro["done"][T - 1].clone()
        A.gae(ro["reward"], ro["done"], ro["values"], ro["last_value"], gamma, gae_lambda, out=(ro["advantages"], ro["returns"]))
        return ro


class LstmPolicy(_LstmRows, torch.nn.Module):
    def __init__(self, weights=None, lstm_hidden_size=256, net_arch=None, activation_fn="tanh", n_rows=None, seed=0, backend="auto",
                 n_lstm_layers=1, shared_lstm=False, enable_critic_lstm=True):
        super().__init__()
        self.backend = backend          # "auto": HIP kernels for CUDA float32 observations, PyTorch otherwise; "torch"; "hip"
        self.noise_seed = int(seed)
        self.noise_env_offset = 0
        self._calls = 0
        self._hip, self._hip_critic = {}, {}        # device index -> rdv_policy handle (each owns the state of n_rows rows)
        self.activation = parse_activation(activation_fn)
        self._fn = ACTIVATIONS[self.activation][1]
        if weights is not None:
            if any(k.startswith("lstm_actor.") and not k.endswith("_l0") for k in weights):
                raise ValueError("the weights hold more than one LSTM layer (lstm_actor.*_l1): n_lstm_layers = 1 is served")
            if "lstm_actor.weight_hh_l0" not in weights:
                raise KeyError("lstm_actor.weight_hh_l0: the weights hold no actor LSTM")
            if "lstm_critic.weight_hh_l0" not in weights:
                raise ValueError("the weights hold no lstm_critic.*: a shared LSTM (shared_lstm = True) or a critic without an LSTM "
                                 "(enable_critic_lstm = False) is not served")
            lstm_hidden_size = int(np.asarray(weights["lstm_actor.weight_hh_l0"]).shape[1])
        check_lstm_config(lstm_hidden_size, n_lstm_layers, shared_lstm, enable_critic_lstm)
        self.lstm_hidden_size = H = int(lstm_hidden_size)
        if net_arch is not None:
            pi, vf = parse_net_arch(net_arch)
        elif weights is not None:
            pi = infer_arch(weights, "policy_net")
            if pi is None:
                raise KeyError("mlp_extractor.policy_net.0.weight: the weights hold no actor trunk")
            vf = infer_arch(weights, "value_net") or pi
            parse_net_arch(dict(pi=pi, vf=vf))
        else:
            pi = vf = [64, 64]
        self.pi_arch, self.vf_arch = list(pi), list(vf)
        self.lstm_actor = torch.nn.LSTM(17, H, num_layers=1)
        self.lstm_critic = torch.nn.LSTM(17, H, num_layers=1)
        for prefix, arch, out in (("l", self.pi_arch, 6), ("v", self.vf_arch, 1)):
            dims = [H] + arch + [out]
            for i in range(len(dims) - 1):
                setattr(self, f"{prefix}{i + 1}", torch.nn.Linear(dims[i], dims[i + 1]))
        self.log_std = torch.nn.Parameter(torch.zeros(6))
        self.has_critic = True
        if weights is not None:
            self._load_weights(weights)
        for p in self.parameters():
            p.requires_grad_(False)
        self.n_rows = None if n_rows is None else int(n_rows)
        self._state = {}                # torch backend: "l" / "v" -> [h, c] once the rows are known
        # the pending episode-start flags of the PyTorch path, and of the time before a HIP handle exists: True (every row, as created),
        # False (none) or the uint8 [rows] tensor a rollout left (done[T-1]).  A HIP handle's flags are mirrored on ITS device, in
        # _dev_pending[(prefix, device index)]: one uint8 [rows] tensor, written in place (_LstmRows._device_flags)
        self._pending = {"l": True, "v": True}
        self._dev_pending = {}

    # ------------------------------------------------------------------------------------------------ weights
    def _layers(self, prefix):
        return [getattr(self, f"{prefix}{i + 1}") for i in range(len(self.pi_arch if prefix == "l" else self.vf_arch) + 1)]

    def _lstm(self, prefix):
        return self.lstm_actor if prefix == "l" else self.lstm_critic

    def _load_weights(self, weights):
        """sb3-contrib's state-dict keys into the modules; every shape is checked before anything is copied."""
        todo = []

        def take(dst, key):
            src = torch.as_tensor(np.asarray(weights[key]), dtype=torch.float32)
            if src.shape != dst.shape:
                raise ValueError(f"{key}: shape {tuple(src.shape)} does not fit the architecture (expected {tuple(dst.shape)})")
            todo.append((dst, src))
        for name, prefix, trunk in (("lstm_actor", "l", "policy_net"), ("lstm_critic", "v", "value_net")):
            for k in _LSTM_KEYS:
                take(getattr(self._lstm(prefix), k), f"{name}.{k}")
            for lin, (kw, kb) in zip(self._layers(prefix), _trunk_keys(trunk, len(self.pi_arch if prefix == "l" else self.vf_arch))):
                take(lin.weight, kw)
                take(lin.bias, kb)
        take(self.log_std, "log_std")
        with torch.no_grad():
            for dst, src in todo:
                dst.copy_(src)

    def state_dict_sb3(self):
        """The parameters under sb3-contrib's keys, as NumPy arrays (what ``__init__`` takes)."""
        out = {"log_std": self.log_std.detach().cpu().numpy()}
        for name, prefix, trunk in (("lstm_actor", "l", "policy_net"), ("lstm_critic", "v", "value_net")):
            for k in _LSTM_KEYS:
                out[f"{name}.{k}"] = getattr(self._lstm(prefix), k).detach().cpu().numpy()
            arch = self.pi_arch if prefix == "l" else self.vf_arch
            for lin, (kw, kb) in zip(self._layers(prefix), _trunk_keys(trunk, len(arch))):
                out[kw], out[kb] = lin.weight.detach().cpu().numpy(), lin.bias.detach().cpu().numpy()
        return out

    @classmethod
    def from_npz(cls, path, **kwargs):
        w = dict(np.load(path, allow_pickle=False))
        if "activation_fn" in w:
            kwargs.setdefault("activation_fn", str(w.pop("activation_fn")))
        return cls(w, **kwargs)

    @classmethod
    def from_sb3_zip(cls, path, **kwargs):
        """An sb3-contrib checkpoint zip as ``model.save()`` writes it; policy.pth is read with weights_only=True (nothing is
        unpickled); H and the trunk come from the shapes, the activation from the zip's ``data`` JSON (absent: tanh)."""
        with zipfile.ZipFile(path) as z:
            sd = torch.load(io.BytesIO(z.read("policy.pth")), weights_only=True, map_location="cpu")
            if "activation_fn" not in kwargs and "data" in z.namelist():
                pk = json.loads(z.read("data").decode("utf-8")).get("policy_kwargs") or {}
                fn = pk.get("activation_fn") if isinstance(pk, dict) else None
                if fn is not None:
                    kwargs["activation_fn"] = parse_activation(fn)
        return cls({k: v.numpy() for k, v in sd.items()}, **kwargs)

    # ------------------------------------------------------------------------------------------------ handles
    def _host_arrays(self, prefix):
        host = lambda t: t.detach().to("cpu", torch.float32).contiguous()
        lstm = self._lstm(prefix)
        layers = self._layers(prefix)
        return ([host(getattr(lstm, k)) for k in _LSTM_KEYS], [host(l.weight) for l in layers], [host(l.bias) for l in layers],
                [host(self.log_std)] if prefix == "l" else [])

    def _create_handle(self, prefix, idx):
        from . import _native as N
        arch = self.pi_arch if prefix == "l" else self.vf_arch
        spec = N.LstmSpec.make(self.lstm_hidden_size, arch, ACTIVATIONS[self.activation][0])
        N.check(N.lib().rdv_lstm_spec_check(C.byref(spec)))
        lstm, ws, bs, log_std = self._host_arrays(prefix)
        wp, bp = _ptrs(ws), _ptrs(bs)
        h = C.c_void_p()
        lp = [C.c_void_p(t.data_ptr()) for t in lstm]
        if prefix == "l":
            N.check(N.lib().rdv_lstm_policy_create(C.byref(spec), *lp, wp, bp, C.c_void_p(log_std[0].data_ptr()), self.n_rows, idx, C.byref(h)))
        else:
            N.check(N.lib().rdv_lstm_critic_create(C.byref(spec), *lp, wp, bp, self.n_rows, idx, C.byref(h)))
        return h

    # ------------------------------------------------------------------------------------------------ evaluation
    def _cell_torch(self, prefix, obs, start, commit=True):
        """One step of the PyTorch modules on [n, 17] observations: the latent h' (the state advances when ``commit``)."""
        st = self._torch_state(prefix, obs.device)
        keep = 1.0 - (torch.zeros(obs.shape[0], device=obs.device) if start is None else start.to(obs.device, torch.float32))
        h0, c0 = st[0] * keep[:, None], st[1] * keep[:, None]
        _, (h1, c1) = self._lstm(prefix)(obs[None].to(torch.float32), (h0[None], c0[None]))
        if commit:
            st[0].copy_(h1[0]); st[1].copy_(c1[0])
            self._pending[prefix] = False
        return h1[0]

    def _trunk_torch(self, prefix, x):
        layers = self._layers(prefix)
        for lin in layers[:-1]:
            x = self._fn(lin(x))
        return layers[-1](x)

    @property
    def _module_device(self):
        return self.log_std.device

    def _forward_torch(self, prefix, obs, start, commit=True):
        return self._trunk_torch(prefix, self._cell_torch(prefix, obs, start, commit=commit))

    def _sample_torch(self, mean, deterministic, generator, log_prob_out):
        a = mean
        if not deterministic:
            noise = torch.randn(a.shape, dtype=a.dtype, device=a.device, generator=generator)
            a = a + torch.exp(self.log_std) * noise
            if log_prob_out is not None:
                log_prob_out.copy_((-0.5 * noise * noise - self.log_std).sum(dim=1) - 3.0 * float(np.log(2.0 * np.pi)))
        elif log_prob_out is not None:
            log_prob_out.fill_(-float(self.log_std.sum()) - 3.0 * float(np.log(2.0 * np.pi)))
        return a

    def predict(self, observation, state=None, episode_start=None, deterministic=True):
        """SB3's calling convention (save_new_trajectory.py:106): NumPy observations [n, 17] (or [17]); ``state`` = the ``(h, c)`` a
        previous call returned (None: the policy's own, zero at first) -> ``(action, state)``."""
        dev = self.log_std.device
        obs = torch.as_tensor(np.asarray(observation), dtype=torch.float32, device=dev)
        single = obs.dim() == 1
        obs = obs.reshape(-1, 17)
        self._rows(obs.shape[0])
        if state is not None:
            self._set_state("l", tuple(torch.as_tensor(np.asarray(s), dtype=torch.float32, device=dev).reshape(obs.shape[0], -1) for s in state))
        a = self.act(obs, episode_start=episode_start, deterministic=deterministic).cpu().numpy()
        h, c = self._get_state("l", dev)
        return (a[0] if single else a), (h.cpu().numpy(), c.cpu().numpy())

    def ppo_grad(self, *args, **kwargs):
        """Not offered for a recurrent policy: ``MlpPolicy.ppo_grad`` serves the feed-forward shipped actor and critic."""
        from . import ppo
        return ppo.ppo_grad(self, *args, **kwargs)

    def ppo_sequence_grad(self, buf, envs=None, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, check=True, state0=None,
                          critic_state0=None):
        """The PPO loss of one minibatch of whole env columns of a recurrent rollout and its gradients, back-propagated through time —
        the body of sb3-contrib's ``RecurrentPPO.train()`` loop for a minibatch that falls on env boundaries (``clip_range_vf=None``).
        ``buf``: what ``RendezvousBatch.collect(policy, T)`` returns.  ``envs``: a 1-d int64 tensor of columns (``ppo_sequence_minibatches``
        yields them), None for all.  Each column starts from ``buf["lstm_state0"]`` / ``buf["lstm_critic_state0"]`` (``state0=`` /
        ``critic_state0=`` override them: pairs ``(h, c)`` of [N, H]), a constant of the minibatch; ``done[t-1]`` resets the state in front
        of step t and cuts the gradient there.  Advantages are normalised with SB3's expression over the T * B entries of the minibatch.
        Fills ``.grad`` of every parameter — both LSTMs, both trunks, ``log_std`` — as views of two flat buffers the policy owns, and
        returns the six scalars as 0-dim tensors plus ``log_prob`` and ``values`` [T, B] of the current networks.  CUDA rows: ONE call of
        rdv_lstm_ppo_loss_grad (include/rdv.h "Recurrent PPO minibatch gradients"; hand-written MFMA kernels, 4 T + 8 launches on the
        current stream, legal inside a stream capture; the policy's state and pending flags are untouched).  CPU rows or
        ``backend="torch"``: float32 autograd through the modules over the T steps, with the same masking."""
        from . import ppo
        return ppo.ppo_sequence_grad(self, buf, envs, clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef,
                                     normalize_advantage=normalize_advantage, check=check, state0=state0, critic_state0=critic_state0)

    def adam_step(self, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5):
        """What follows ``ppo_sequence_grad``: ``LstmPolicySet.sequence_adam_step`` on this policy as a set of one — behind a
        ``ppo_sequence_grad`` that ran rdv_lstm_ppo_loss_grad, ONE rdv_lstm_ppo_set_adam_step on the plain handle pair, on the buffers
        that call filled (the parameters become views of a master row the policy owns; no ``update_weights()`` is needed); otherwise
        ``clip_grad_norm_`` and a ``torch.optim.Adam`` the policy owns, and ``update_weights()`` follows.  Returns the dict of [1]
        tensors ``total_norm``, ``clip_coef``, ``skipped``."""
        from . import ppo
        return ppo.lstm_adam_step(self, None, lr, betas, eps, max_grad_norm)

    sequence_adam_step = adam_step       # the name the set gives it

    def reset_optimizer(self):
        """Zero the Adam moments and the step counter (device state and fallback optimiser alike); the weights are not touched."""
        from . import ppo
        return ppo.set_reset_optimizer(self, None)

    def update_weights(self, weights=None):
        """New weights for the modules (a dict with the constructor's keys; None: push the modules' current parameters) and for every
        live HIP handle, through rdv_lstm_set_weights on the current stream of its device; the recurrent state is kept."""
        if weights is not None:
            self._load_weights(weights)
        self._refresh_handles()

    def _refresh(self, h, prefix, member, stream):
        """rdv_lstm_set_weights, or rdv_lstm_set_member_weights as block ``member`` of a set handle: h <- this policy's LSTM and trunk."""
        from . import _native as N
        lstm, ws, bs, log_std = self._host_arrays(prefix)
        args = (*[C.c_void_p(t.data_ptr()) for t in lstm], _ptrs(ws), _ptrs(bs), C.c_void_p(log_std[0].data_ptr()) if log_std else None, stream)
        N.check(N.lib().rdv_lstm_set_weights(h, *args) if member is None else N.lib().rdv_lstm_set_member_weights(h, member, *args))


class LstmPolicySet(_Members, _LstmRows):
    """P recurrent member policies of ONE architecture over one batch: member g owns the next ``group_sizes[g]`` rows, and one cell launch
    and one trunk launch per call evaluate all members (include/rdv.h, "Recurrent policy sets"; csrc/rdv_policy_lstm.h) — what
    ``PolicySet`` is for MLP learners.  Row i of member g gets bit for bit what a stand-alone ``LstmPolicy`` of member g's weights with
    ``n_rows = group_sizes[g]`` computes for that row, fed the same observations and episode starts, with the same noise seed, the same
    call counter and ``env_id_offset + start_g`` — actions, samples, log-densities, values, and the state after every call.

    ``policies``: ``LstmPolicy`` modules with the same ``lstm_hidden_size``, ``pi_arch``, ``vf_arch`` and ``activation`` (ValueError naming
    the member and the field).  They stay the source of truth for the weights (``set[g]``); their own ``n_rows`` and state are not used:
    the SET owns the state of all rows (``state``, ``critic_state``, ``reset_state``, ``state_at_start``) and the pending episode-start
    flags.  ``group_sizes``: positive, every one but the last a multiple of 256 rows — the rule and the messages of
    rdv_param_groups_check, checked on the host.  ``RendezvousBatch.rollout`` / ``collect`` take a set where they take an ``LstmPolicy``;
    the set's ranges and the batch's parameter groups are independent.  One noise key for the whole set (``seed``) and one call counter.
    CUDA float32 input goes to the set kernels; CPU input or ``backend="torch"`` loops the members' modules over their slices."""

    _refresh_call = "rdv_lstm_set_member_weights"

    def __init__(self, policies, group_sizes, seed=0, backend="auto"):
        self._init_members("LstmPolicySet", LstmPolicy, ("lstm_hidden_size", "pi_arch", "vf_arch", "activation"), policies, group_sizes)
        self.n_rows = self.num_rows
        self.backend = backend
        self.noise_seed = int(seed)
        self.noise_env_offset = 0
        self._calls = 0
        self._hip, self._hip_critic = {}, {}        # device index -> rdv_policy handle of the set (each owns the state of all rows)
        self.has_critic = True
        self._state = {}
        self._pending = {"l": True, "v": True}
        self._dev_pending = {}

    # ------------------------------------------------------------------------------------------------ handles
    def _create_handle(self, prefix, idx):
        """rdv_lstm_policy_set_create / rdv_lstm_critic_set_create from the members' modules."""
        from . import _native as N
        arch = self.pi_arch if prefix == "l" else self.vf_arch
        spec = N.LstmSpec.make(self.lstm_hidden_size, arch, ACTIVATIONS[self.activation][0])
        N.check(N.lib().rdv_lstm_spec_check(C.byref(spec)))
        host = [p._host_arrays(prefix) for p in self.policies]        # kept alive until the call returns
        P, sizes, wpp, bpp, lsp = self._member_tables(host)
        lstm = [_ptrs([m[0][k] for m in host]) for k in range(len(_LSTM_KEYS))]
        h = C.c_void_p()
        if prefix == "l":
            N.check(N.lib().rdv_lstm_policy_set_create(C.byref(spec), P, sizes, *lstm, wpp, bpp, lsp, idx, C.byref(h)))
        else:
            N.check(N.lib().rdv_lstm_critic_set_create(C.byref(spec), P, sizes, *lstm, wpp, bpp, idx, C.byref(h)))
        return h

    # ------------------------------------------------------------------------------------------------ the PyTorch path
    @property
    def _module_device(self):
        return self.policies[0].log_std.device

    def _forward_torch(self, prefix, obs, start, commit=True):
        """One step of the members' modules, each on its slice of the set's state."""
        st = self._torch_state(prefix, obs.device)
        keep = 1.0 - (torch.zeros(obs.shape[0], device=obs.device) if start is None else start.to(obs.device, torch.float32))
        outs = []
        for p, s in zip(self.policies, self.group_slices):
            h0, c0 = st[0][s] * keep[s, None], st[1][s] * keep[s, None]
            _, (h1, c1) = p._lstm(prefix)(obs[s][None].to(torch.float32), (h0[None], c0[None]))
            if commit:
                st[0][s].copy_(h1[0]); st[1][s].copy_(c1[0])
            outs.append(p._trunk_torch(prefix, h1[0]))
        if commit:
            self._pending[prefix] = False
        return torch.cat(outs, dim=0)

    def _sample_torch(self, mean, deterministic, generator, log_prob_out):
        return torch.cat([p._sample_torch(mean[s], deterministic, generator, None if log_prob_out is None else log_prob_out[s])
                          for p, s in zip(self.policies, self.group_slices)], dim=0)

    # ------------------------------------------------------------------------------------------------ weights
    def ppo_grad(self, *args, **kwargs):
        """Not offered for a recurrent policy: ``MlpPolicy.ppo_grad`` serves the feed-forward shipped actor and critic."""
        from . import ppo
        return ppo.ppo_grad(self, *args, **kwargs)

    def ppo_grads(self, *args, **kwargs):
        """Not offered for a recurrent set: ``PolicySet.ppo_grads`` serves sets of the feed-forward shipped actor and critic
        (``ppo_sequence_grads`` is the recurrent set's)."""
        from . import ppo
        return ppo.ppo_set_grads(self, *args, **kwargs)

    def ppo_sequence_grads(self, buf, pieces, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, check=True):
        """``LstmPolicy.ppo_sequence_grad`` for every member at once: member g's minibatch is the whole env columns ``pieces[g]`` (a 1-d
        int64 tensor of GLOBAL columns inside ``group_slices[g]``; ``None``: the member sits the call out; a duplicate counts once per
        occurrence; ``ppo_sequence_set_minibatches`` yields such lists) of ``buf``, what ``RendezvousBatch.collect(set, T)`` returns with
        ``N == num_rows``.  Each member's advantages are normalised with SB3's expression over its own T * B_g entries.  Fills ``.grad``
        of every parameter of every present member, as views of member g's rows of [P, Ga] and [P, Gc] buffers the set owns, and returns
        a list of P dicts (``None`` for absent members): the six scalars as 0-dim tensors plus ``log_prob`` and ``values`` [T, B_g].
        CUDA rows: ONE call of rdv_lstm_ppo_set_loss_grad (include/rdv.h "Recurrent PPO minibatch gradients for recurrent sets"): the
        members share 4 T + 8 launches, and every member gets the bits of a stand-alone ``LstmPolicy.ppo_sequence_grad`` with its
        weights on the same buffer.  CPU rows or ``backend="torch"``: the members' own autograd fallback one by one.  ``sequence_adam_step``
        is what follows: clip, Adam and the refresh of the members' forward blocks, on the device behind a call that took the C path."""
        from . import ppo
        return ppo.ppo_sequence_set_grads(self, buf, pieces, clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef,
                                          normalize_advantage=normalize_advantage, check=check)

    def sequence_adam_step(self, stepped=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5):
        """``PolicySet.adam_step`` for a recurrent set (named beside ``ppo_sequence_grads``; the set has no method called ``adam_step``) — what follows ``ppo_sequence_grads`` in a learner's step, for every member at
        once: ``clip_grad_norm_`` per member over both LSTMs, both trunks and ``log_std`` under ONE norm, ``torch.optim.Adam(eps=eps)``
        and the refresh of the members' forward blocks.  ``stepped``: the list ``ppo_sequence_grads`` returned (a ``None`` entry sits
        out); ``None``: all members step.  Same semantics and return value as ``PolicySet.adam_step``.

        Behind a ``ppo_sequence_grads`` that ran rdv_lstm_ppo_set_loss_grad (CUDA rows, ``backend != "torch"``, at most 64 members):
        ONE rdv_lstm_ppo_set_adam_step on the current stream (include/rdv.h "Gradient clip, Adam and weight repack for recurrent policy
        sets"; four launches whatever P, no allocation past the first use, no synchronisation, no host copy, legal inside a stream
        capture, each replay taking the next step).  On first use the set allocates master weights [P,Ga] / [P,Gc], moments, step
        counters, coef and the workspace on that device and re-points every parameter of every member — the ``nn.LSTM`` weights
        included — at views of row g, in the order of the gradient rows; ``.grad`` stays bound to the gradient rows.  NO
        ``update_weights()`` is needed: the call rewrites the members' blocks [trunk | cell] with the bytes ``update_weights`` would
        pack, but for the six ``exp(log_std)`` floats of an actor block (within 1 ulp of the correctly rounded float, within 2 ulp of the
        host packer's; deterministic actions, values and the state do not read them).  A member with a non-finite norm is skipped whole.
        The set's state (h, c) and pending flags are untouched.

        CPU rows, ``backend="torch"`` or more than 64 members: per-member ``clip_grad_norm_`` and one ``torch.optim.Adam`` over all
        members' parameters, as ``PolicySet.adam_step`` falls back; ``update_weights()`` then follows as before."""
        from . import ppo
        return ppo.lstm_adam_step(self, stepped, lr, betas, eps, max_grad_norm)

    def reset_optimizer(self, member=None):
        """Zero the Adam moments and the step counter of one member or of all (None), on the device state and in the fallback's
        optimiser alike; the weights are not touched (``PolicySet.reset_optimizer``)."""
        from . import ppo
        return ppo.set_reset_optimizer(self, member)
