"""
The SB3 MlpPolicy actor of the reference's shipped checkpoint (models/mlp_model_best.zip -> policy.pth):
``a = clip(W3 tanh(W2 tanh(W1 obs + b1) + b2) + b3, -1, 1)``, 17-64-64-6, float32, plus the stochastic rollout form
``a = clip(mean + exp(log_std) * N(0,1), -1, 1)`` that SB3's collect_rollouts uses (main.py:33-46 builds it with
``activation_fn=Tanh``).  It is not part of the env kernel.  On the GPU the forward pass is ONE hand-written HIP kernel
(csrc/rdv_policy.h, through the C ABI: rdv_policy_act); ``backend="torch"`` keeps the plain PyTorch modules (any device),
which the tests use as the reference of that kernel.

Other architectures of the reference's network sweep (tune_policy.py:30-34, :131-139: ``net_arch = [n_neurons] * n_layers``,
``activation_fn`` in ReLU / Sigmoid / Tanh; custom/custom_networks.py:9-10: ReLU, [32, 32]) are held the same way: separate actor
and critic trunks of 1..4 hidden layers, one activation for the whole network.  Their HIP kernels are csrc/rdv_policy_mlp.h
(rdv_policy_create_mlp: widths 16, 32 and 64); the PyTorch modules hold any width.
"""
import ctypes as C
import io
import json
import re
import zipfile

import numpy as np
import torch

_KEYS = ["mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias", "mlp_extractor.policy_net.2.weight",
         "mlp_extractor.policy_net.2.bias", "action_net.weight", "action_net.bias", "log_std"]
_VKEYS = ["mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias", "mlp_extractor.value_net.2.weight",
          "mlp_extractor.value_net.2.bias", "value_net.weight", "value_net.bias"]     # the critic trunk + head of the same checkpoint

ACTIVATIONS = {"tanh": (0, torch.tanh, torch.nn.Tanh), "relu": (1, torch.relu, torch.nn.ReLU),
               "sigmoid": (2, torch.sigmoid, torch.nn.Sigmoid)}       # name -> (RdvActivation, function, SB3's activation_fn class)
MAX_HIDDEN = 4                                                          # RDV_MLP_MAX_HIDDEN


def parse_activation(fn):
    """"tanh" | "relu" | "sigmoid" (any case), the torch.nn class, or the class's string form as an SB3 zip's `data` JSON
    carries it ("<class 'torch.nn.modules.activation.ReLU'>") -> the name."""
    if isinstance(fn, type):
        for name, (_, _, cls) in ACTIVATIONS.items():
            if fn is cls:
                return name
        raise ValueError(f"activation_fn {fn!r} is not supported: one of torch.nn.Tanh, torch.nn.ReLU, torch.nn.Sigmoid")
    text = str(fn)
    m = re.fullmatch(r"<class '([\w.]+)'>", text.strip())
    name = (m.group(1).rsplit(".", 1)[-1] if m else text.strip()).lower()
    if name not in ACTIVATIONS or (m and not m.group(1).startswith("torch.nn.")):
        raise ValueError(f"activation_fn {text!r} is not supported: one of 'tanh', 'relu', 'sigmoid' (or the torch.nn class)")
    return name


def parse_net_arch(net_arch):
    """SB3's net_arch -> (pi, vf): a list of widths (the same for actor and critic), dict(pi=[...], vf=[...]), or the older
    [dict(pi=..., vf=...)].  A shared trunk ([128, dict(...)]) is refused: the kernels hold separate trunks, as SB3 >= 1.8 does."""
    if isinstance(net_arch, dict):
        pi, vf = net_arch.get("pi", []), net_arch.get("vf", [])
    else:
        net_arch = list(net_arch)
        if len(net_arch) == 1 and isinstance(net_arch[0], dict):
            return parse_net_arch(net_arch[0])
        if any(isinstance(x, dict) for x in net_arch):
            raise ValueError(f"net_arch {net_arch!r} has a shared trunk in front of the pi / vf heads: not supported "
                             "(separate actor and critic trunks only)")
        pi = vf = net_arch
    pi, vf = [int(x) for x in pi], [int(x) for x in vf]
    for name, arch in (("pi", pi), ("vf", vf)):
        if not 1 <= len(arch) <= MAX_HIDDEN or min(arch) <= 0:
            raise ValueError(f"net_arch {name} = {arch!r}: 1..{MAX_HIDDEN} hidden layers of positive width")
    return pi, vf


def _trunk_keys(net, n_hidden):
    """The state-dict keys of a trunk of n_hidden layers ('policy_net' + action_net, or 'value_net' + value_net) in layer order."""
    head = "action_net" if net == "policy_net" else "value_net"
    names = [f"mlp_extractor.{net}.{2 * l}" for l in range(n_hidden)] + [head]
    return [(f"{n}.weight", f"{n}.bias") for n in names]


def infer_arch(weights, net):
    """Hidden widths from the keys mlp_extractor.<net>.{0,2,4,6}.weight and their shapes; None when the weights hold none."""
    arch = []
    while f"mlp_extractor.{net}.{2 * len(arch)}.weight" in weights:
        arch.append(int(np.asarray(weights[f"mlp_extractor.{net}.{2 * len(arch)}.weight"]).shape[0]))
    return arch or None


@torch.no_grad()
def _advantages(policy, ro, gamma, gae_lambda, out):
    """``MlpPolicy.advantages`` / ``PolicySet.advantages``: ``policy`` gives has_critic, backend, _critic_handle(device) and
    _value_torch(obs)."""
    from . import advantages as A
    if not policy.has_critic:
        raise ValueError("advantages: this policy has no critic (its weights hold no value_net trunk)")
    obs = ro["obs"]
    if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[2] != 17:
        raise ValueError(f"obs: expected a [T,N,17] tensor, got {tuple(getattr(obs, 'shape', ()))}")
    T, n, dev = int(obs.shape[0]), int(obs.shape[1]), obs.device
    A.check_tensor(obs, "obs", (T, n, 17), torch.float32, dev)
    A.check_tensor(ro["reward"], "reward", (T, n), torch.float32, dev)
    A.check_tensor(ro["done"], "done", (T, n), torch.uint8, dev)
    A.check_tensor(ro["last_obs"], "last_obs", (n, 17), torch.float32, dev)
    A.check_discounts(gamma, gae_lambda)
    cols = dict(values=(T, n), last_value=(n,), advantages=(T, n), returns=(T, n))
    src = out if out is not None else ro
    for name, shape in cols.items():
        t = src.get(name)
        if t is None or tuple(t.shape) != shape or t.device != dev:
            t = torch.empty(shape, dtype=torch.float32, device=dev)
        A.check_tensor(t, name, shape, torch.float32, dev)
        ro[name] = t
    if policy.backend != "torch" and obs.is_cuda:
        from . import _native as N
        rows = N.RolloutOut(obs.data_ptr(), None, ro["reward"].data_ptr(), ro["done"].data_ptr(), None, ro["last_obs"].data_ptr())
        ao = N.AdvantageOut(*[ro[f].data_ptr() for f, _ in N.AdvantageOut._fields_])
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        N.check(N.lib().rdv_rollout_advantages(policy._critic_handle(dev), C.byref(rows), T, n, float(gamma), float(gae_lambda),
                                               C.byref(ao), stream))
        return ro
    ro["values"].copy_(policy._value_torch(obs))
    ro["last_value"].copy_(policy._value_torch(ro["last_obs"]))
    A.gae(ro["reward"], ro["done"], ro["values"], ro["last_value"], gamma, gae_lambda, out=(ro["advantages"], ro["returns"]))
    return ro


def _ptrs(tensors):
    """A C array of the tensors' addresses, as the ABI's ``const float* const*`` arguments take them (the tensors outlive the call)."""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _pptrs(lists):
    """``const float* const* const*``: a C array of the addresses of one ``_ptrs`` array per list of tensors (which it keeps alive)."""
    rows = [_ptrs(ts) for ts in lists]
    out = (C.c_void_p * len(rows))(*[C.addressof(a) for a in rows])
    out._rows = rows
    return out


class _HipHandles:
    """The HIP side that MlpPolicy, PolicySet and LstmPolicy share: the per-device handle caches ``_hip`` (actor) and ``_hip_critic``
    (device index -> rdv_policy, made on first use by the class's ``_create_handle(prefix, idx)``; prefix "l": actor, "v": critic),
    ``close``, the weight refresh of the live handles, and the rdv_policy_act / rdv_policy_value calls of the feed-forward handles."""

    @staticmethod
    def _stream(device):
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def _refresh_handles(self, members=(None,)):
        """THE loop of every ``update_weights``: each live actor and critic handle, on the current stream of its device, through the
        class's ``_refresh(h, prefix, member, stream)`` (handle h <- the modules' trunk ``prefix``; ``member``: the block of a set handle
        and the member whose modules are read, None for a policy of its own)."""
        for prefix, handles in (("l", self._hip), ("v", self._hip_critic)):
            for g in members:
                for idx, h in handles.items():
                    self._refresh(h, prefix, g, self._stream(torch.device("cuda", idx)))

    def _handle(self, prefix, device):
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        table = self._hip if prefix == "l" else self._hip_critic
        if idx not in table:
            table[idx] = self._create_handle(prefix, idx)
        return table[idx]

    def _hip_handle(self, device):
        return self._handle("l", device)

    def _critic_handle(self, device):
        return self._handle("v", device)

    def close(self):
        if self._hip or self._hip_critic:
            from . import _native as N
            for h in list(self._hip.values()) + list(self._hip_critic.values()):
                N.lib().rdv_policy_destroy(h)
            self._hip, self._hip_critic = {}, {}

    def _act_hip(self, obs, deterministic, out=None, env_id_offset=None):
        """rdv_policy_act on the actor handle of the rows' device, current stream; the call counter advances."""
        from . import _native as N
        offset = self.noise_env_offset if env_id_offset is None else int(env_id_offset)
        obs = obs.contiguous()
        n = obs.shape[0]
        if out is None:
            out = torch.empty((n, 6), dtype=torch.float32, device=obs.device)
        N.check(N.lib().rdv_policy_act(self._hip_handle(obs.device), C.c_void_p(obs.data_ptr()), C.c_void_p(out.data_ptr()), n,
                                       int(bool(deterministic)), C.c_uint64(self.noise_seed), C.c_uint64(self._calls),
                                       C.c_uint64(offset), self._stream(obs.device)))
        self._calls += 1
        return out

    def _value_hip(self, obs, out=None):
        """rdv_policy_value on the critic handle: float32 CUDA observations [..., 17] -> values [...], current stream."""
        from . import _native as N
        flat = obs.reshape(-1, 17).contiguous()
        if out is None:
            out = torch.empty((flat.shape[0],), dtype=torch.float32, device=flat.device)
        N.check(N.lib().rdv_policy_value(self._critic_handle(flat.device), C.c_void_p(flat.data_ptr()), C.c_void_p(out.data_ptr()),
                                         flat.shape[0], self._stream(flat.device)))
        return out.reshape(obs.shape[:-1])


class _Members:
    """Set membership, which PolicySet and LstmPolicySet share: P member policies of ONE architecture, member g owning rows
    ``group_slices[g]`` (the next ``group_sizes[g]``) of ``num_rows``, held in ``policies``; the container protocol, the ctypes member
    tables of the set-create calls, and ``update_weights``.  The class gives ``_refresh_call``, the ABI function that the members'
    ``_refresh`` reaches for a block of a set handle."""

    def _init_members(self, name, member_type, fields, policies, group_sizes, num_rows=None):
        """The validation at construction: ``name`` is the class's in the messages, ``fields`` what the members must agree in (the set
        takes them from member 0).  The sizes: the rule and the messages of rdv_param_groups_check (params.group_tile_table)."""
        from .params import group_tile_table
        policies = list(policies)
        if not policies:
            raise ValueError(f"{name}: at least one member policy")
        sizes = [int(x) for x in group_sizes]
        if len(sizes) != len(policies):
            raise ValueError(f"{name}: {len(policies)} policies but {len(sizes)} group sizes")
        first = policies[0]
        for g, p in enumerate(policies):
            if not isinstance(p, member_type):
                raise TypeError(f"{name}: member {g} is a {type(p).__name__}, not an {member_type.__name__}")
            for what in fields:
                if getattr(p, what) != getattr(first, what):
                    raise ValueError(f"{name}: member {g} has {what} = {getattr(p, what)!r}, member 0 has {getattr(first, what)!r}: "
                                     "the members of a set share one architecture")
        rows = sum(sizes) if num_rows is None else int(num_rows)
        group_tile_table(rows, sizes)
        self.policies, self.group_sizes, self.num_rows = policies, sizes, rows
        starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.group_slices = [slice(int(starts[g]), int(starts[g + 1])) for g in range(len(sizes))]
        for what in fields:
            v = getattr(first, what)
            setattr(self, what, list(v) if isinstance(v, list) else v)

    def __len__(self):
        return len(self.policies)

    def __getitem__(self, g):
        return self.policies[g]

    def __iter__(self):
        return iter(self.policies)

    def to(self, *args, **kwargs):
        """The member modules moved as ``torch.nn.Module.to`` moves them (the HIP handles live on the device of the rows they are given)."""
        self.policies = [p.to(*args, **kwargs) for p in self.policies]
        return self

    def _member_tables(self, host):
        """(P, sizes, weights, biases, log_std) as the set-create calls take them; ``host[g][-3:]``: member g's (weights, biases,
        [log_std] or []) on the host, which the caller keeps alive until the call returns."""
        sizes = (C.c_int64 * len(host))(*self.group_sizes)
        return (len(host), sizes, _pptrs([m[-3] for m in host]), _pptrs([m[-2] for m in host]),
                _ptrs([m[-1][0] for m in host]) if host[0][-1] else None)

    def _refresh(self, h, prefix, member, stream):
        self.policies[member]._refresh(h, prefix, member, stream)

    def update_weights(self, member=None, weights=None):
        """New weights for one member (``member`` = its index; ``weights``: a dict as the member's own ``update_weights`` takes, or None
        to push the member module's current parameters) or for all members (``member`` None; ``weights``: None or a list of one dict or
        None per member).  Dicts are loaded into the member modules first; then every live set handle is refreshed member by member
        through rdv_policy_set_member_weights (a recurrent set: rdv_lstm_set_member_weights) on the current stream of its device:
        launches already queued there use the old weights, later ones the new; the other members' blocks, and a recurrent set's state,
        are not touched.  Not legal while the current stream is being captured (RdvError, nothing touched).  The noise key and the call
        counter are unchanged.  (A ``PolicySet`` that has taken an ``adam_step`` on the device: the dicts are written through the members'
        parameters into the master weights the set owns; the optimiser's moments and step counters are kept — ``reset_optimizer``.)"""
        P = len(self.policies)
        if (self._hip or self._hip_critic) and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            # refused before a module or a host copy is touched (either would invalidate the capture); the library refuses the same way
            from . import _native as N
            raise N.RdvError(-1, f"{self._refresh_call}: not legal inside a stream capture (the staging buffer is reused by the next call)")
        if member is None:
            todo = list(range(P))
            per = weights if weights is not None else [None] * P
            if isinstance(per, dict) or len(per) != P:
                raise ValueError(f"update_weights: weights for all members is a list of {P} dicts (or None); pass member= for one")
        else:
            member = int(member)
            if not 0 <= member < P:
                raise IndexError(f"update_weights: member {member} of {P}")
            todo, per = [member], {member: weights}
        for g in todo:
            if per[g] is not None:
                self.policies[g]._load_weights(per[g])
        self._refresh_handles(todo)


class MlpPolicy(_HipHandles, torch.nn.Module):
    def __init__(self, weights=None, net_arch=None, activation_fn="tanh", obs_dim=17, hidden=64, act_dim=6, seed=0, backend="auto"):
        super().__init__()
        self.backend = backend          # "auto": HIP kernel for CUDA observations, PyTorch otherwise; "torch"; "hip"
        self.noise_seed = int(seed)     # HIP backend: Philox key of the exploration noise; the call counter is the step index
        self.noise_env_offset = 0       # HIP backend: global index of row 0 when act() is not told (sharded batches key the noise by
                                        # GLOBAL env id: RendezvousBatch.act / .rollout pass the shard's env_id_offset themselves)
        self._hip = {}                  # device index -> rdv_policy handle
        self._hip_critic = {}           # device index -> rdv_policy handle of the critic
        self._calls = 0
        self.activation = parse_activation(activation_fn)
        self._fn = ACTIVATIONS[self.activation][1]
        if net_arch is not None:
            pi, vf = parse_net_arch(net_arch)
        elif weights is not None:
            pi = infer_arch(weights, "policy_net")
            if pi is None:
                raise KeyError("mlp_extractor.policy_net.0.weight: the weights hold no actor trunk")
            vf = infer_arch(weights, "value_net") or pi
            parse_net_arch(dict(pi=pi, vf=vf))
        else:
            pi = vf = [hidden, hidden]
        self.pi_arch, self.vf_arch = list(pi), list(vf)
        # actor: l1 .. l<n>, the last one the head (17-64-64-6: l1, l2, l3); critic (SB3 MlpPolicy: a separate trunk + a head of
        # one row): v1 .. v<m>, left at PyTorch's initialisation when the weights have none
        for prefix, arch, out in (("l", self.pi_arch, act_dim), ("v", self.vf_arch, 1)):
            dims = [obs_dim] + arch + [out]
            for i in range(len(dims) - 1):
                setattr(self, f"{prefix}{i + 1}", torch.nn.Linear(dims[i], dims[i + 1]))
            if prefix == "l":
                self.log_std = torch.nn.Parameter(torch.zeros(act_dim))
        self.has_critic = False
        if weights is None:
            # random init of the architecture (bench.py when the checkpoint fixture is absent): SB3's orthogonal gains
            g = torch.Generator().manual_seed(seed)
            actor = self._layers("l")
            for lin, gain in zip(actor, [2 ** 0.5] * (len(actor) - 1) + [0.01]):
                torch.nn.init.orthogonal_(lin.weight, gain=gain, generator=g)
                torch.nn.init.zeros_(lin.bias)
        else:
            self._load_weights(weights)
        for p in self.parameters():
            p.requires_grad_(False)

    def _load_weights(self, weights):
        """The actor's layers and log_std, and the critic's when the weights hold every key of its trunk, into the modules (SB3's
        state-dict keys); a shape that does not fit the architecture raises ValueError."""
        todo = []           # every shape is checked before anything is copied: a refused dict leaves the modules as they were

        def load(layers, keys):
            for lin, (kw, kb) in zip(layers, keys):
                w, b = (torch.as_tensor(np.asarray(weights[k]), dtype=torch.float32) for k in (kw, kb))
                if w.shape != lin.weight.shape or b.shape != lin.bias.shape:
                    raise ValueError(f"{kw}: shape {tuple(w.shape)} does not fit net_arch (expected {tuple(lin.weight.shape)})")
                todo.extend([(lin.weight, w), (lin.bias, b)])
        load(self._layers("l"), _trunk_keys("policy_net", len(self.pi_arch)))
        log_std = torch.as_tensor(np.asarray(weights["log_std"]), dtype=torch.float32)
        if log_std.shape != self.log_std.shape:
            raise ValueError(f"log_std: shape {tuple(log_std.shape)} (expected {tuple(self.log_std.shape)})")
        todo.append((self.log_std, log_std))
        vkeys = _trunk_keys("value_net", len(self.vf_arch))
        critic = all(k in weights for pair in vkeys for k in pair)
        if critic:
            load(self._layers("v"), vkeys)
        with torch.no_grad():
            for dst, src in todo:
                dst.copy_(src)
        self.has_critic = self.has_critic or critic

    def _layers(self, prefix):
        return [getattr(self, f"{prefix}{i + 1}") for i in range(len(self.pi_arch if prefix == "l" else self.vf_arch) + 1)]

    @property
    def shipped_arch(self):
        """The architecture of the shipped checkpoint (actor): the specialised kernels and the one-launch rollout."""
        return self.pi_arch == [64, 64] and self.activation == "tanh" and self.l1.in_features == 17

    @classmethod
    def from_npz(cls, path, **kwargs):
        """Weights extracted from policy.pth as plain arrays (tests/golden/mlp_policy.npz); an optional string entry
        ``activation_fn`` names the activation (absent: tanh)."""
        w = dict(np.load(path, allow_pickle=False))
        if "activation_fn" in w:
            kwargs.setdefault("activation_fn", str(w.pop("activation_fn")))
        return cls(w, **kwargs)

    @classmethod
    def from_sb3_zip(cls, path, **kwargs):
        """An SB3 checkpoint zip as `model.save()` writes it; policy.pth is read with weights_only=True (nothing is unpickled).
        The layers come from policy.pth, the activation from the zip's `data` JSON: policy_kwargs["activation_fn"], the string
        form of the class that SB3 writes beside the pickled blob (absent: SB3's default, tanh)."""
        with zipfile.ZipFile(path) as z:
            sd = torch.load(io.BytesIO(z.read("policy.pth")), weights_only=True, map_location="cpu")
            if "activation_fn" not in kwargs and "data" in z.namelist():
                pk = json.loads(z.read("data").decode("utf-8")).get("policy_kwargs") or {}
                fn = pk.get("activation_fn") if isinstance(pk, dict) else None
                if fn is not None:
                    kwargs["activation_fn"] = parse_activation(fn)
        return cls({k: v.numpy() for k, v in sd.items()}, **kwargs)

    def _forward(self, prefix, x):
        layers = self._layers(prefix)
        for lin in layers[:-1]:
            x = self._fn(lin(x))
        return layers[-1](x)

    @torch.no_grad()
    def mean(self, obs):
        return self._forward("l", obs)

    def _host_layers(self, prefix):
        """(weights, biases, [log_std] or []) of a trunk as contiguous float32 CPU tensors, hidden layers first, the head last."""
        host = lambda t: t.detach().to("cpu", torch.float32).contiguous()
        layers = self._layers(prefix)
        return [host(l.weight) for l in layers], [host(l.bias) for l in layers], [host(self.log_std)] if prefix == "l" else []

    def _create_handle(self, prefix, idx):
        """rdv_policy_create / rdv_critic_create for the shipped architecture, their _mlp forms (RdvMlpSpec) for every other."""
        from . import _native as N
        arch = self.pi_arch if prefix == "l" else self.vf_arch
        ws, bs, log_std = self._host_layers(prefix)
        h = C.c_void_p()
        if arch == [64, 64] and self.activation == "tanh":
            flat = [t for pair in zip(ws, bs) for t in pair] + log_std
            create = N.lib().rdv_policy_create if prefix == "l" else N.lib().rdv_critic_create
            N.check(create(*[C.c_void_p(t.data_ptr()) for t in flat], idx, C.byref(h)))
            return h
        spec = N.MlpSpec.make(arch, ACTIVATIONS[self.activation][0])
        N.check(N.lib().rdv_mlp_spec_check(C.byref(spec)))        # a message naming the field, before any pointer is read
        if prefix == "l":
            N.check(N.lib().rdv_policy_create_mlp(C.byref(spec), _ptrs(ws), _ptrs(bs), C.c_void_p(log_std[0].data_ptr()), idx, C.byref(h)))
        else:
            N.check(N.lib().rdv_critic_create_mlp(C.byref(spec), _ptrs(ws), _ptrs(bs), idx, C.byref(h)))
        return h

    @torch.no_grad()
    def value(self, obs, out=None):
        """The critic's value estimate for observations [..., 17] (SB3 ``policy.predict_values``): one HIP kernel for CUDA
        float32 observations (rdv_policy_value), the PyTorch modules otherwise / with ``backend="torch"``."""
        if self.backend != "torch" and obs.is_cuda and obs.dtype == torch.float32:
            return self._value_hip(obs, out)
        return self._value_torch(obs)

    @torch.no_grad()
    def advantages(self, ro, gamma=0.99, gae_lambda=0.95, out=None):
        """The columns of SB3's RolloutBuffer that a rollout does not hold, for the rows ``ro`` of ``RendezvousBatch.rollout``:
        ``values`` [T,N] (the critic on ``ro["obs"]``), ``last_value`` [N] (on ``ro["last_obs"]``), ``advantages`` and ``returns``
        [T,N] (GAE: ``RolloutBuffer.compute_returns_and_advantage``; the defaults are SB3's).  Returns ``ro`` with the four added.
        They are allocated once: taken from ``out`` (e.g. the dict an earlier call returned), or from ``ro`` itself when it has them.
        CUDA rows: rdv_rollout_advantages on the current stream (two critic launches and the GAE kernel; the values are the critic's
        at call time, bit-identical to ``value()``); ``backend="torch"`` or CPU rows: the modules plus ``advantages.gae``."""
        return _advantages(self, ro, gamma, gae_lambda, out)

    def _value_torch(self, obs):
        """The critic's PyTorch modules on observations [..., 17]."""
        return self._forward("v", obs.reshape(-1, 17)).reshape(obs.shape[:-1])

    def update_weights(self, weights=None):
        """New weights for the policy and for every live HIP handle of it — what a learner calls after ``optimizer.step()``.
        ``weights``: a dict with the constructor's keys, loaded into the modules first (shapes are checked as in ``__init__``; the
        critic is loaded when the dict holds its trunk); ``None``: the modules' current parameters are pushed.  Each actor / critic
        handle is refreshed through rdv_policy_set_weights on the current stream of its device: launches already queued there use the
        old weights, later ones the new.  A non-finite weight raises RdvError (BAD_PARAMS) and leaves that handle as it was.  The
        call counter and the noise key are unchanged."""
        if weights is not None:
            self._load_weights(weights)
        self._refresh_handles()

    def _refresh(self, h, prefix, member, stream):
        """rdv_policy_set_weights, or rdv_policy_set_member_weights as block ``member`` of a set handle: h <- this policy's trunk."""
        from . import _native as N
        ws, bs, log_std = self._host_layers(prefix)
        args = (_ptrs(ws), _ptrs(bs), C.c_void_p(log_std[0].data_ptr()) if log_std else None, stream)
        N.check(N.lib().rdv_policy_set_weights(h, *args) if member is None else N.lib().rdv_policy_set_member_weights(h, member, *args))

    def ppo_grad(self, buf, indices=None, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, check=True):
        """The loss of SB3's ``PPO.train()`` for ONE minibatch and its gradients, written into ``.grad`` of this module's 13 parameters
        (ppo.py; include/rdv.h "PPO minibatch gradients").  ``buf``: the dict ``RendezvousBatch.collect`` returns; its [T,N,...] columns
        ``obs``, ``actions`` (unclipped), ``log_prob`` (the old one), ``advantages`` and ``returns`` are viewed flat, not copied.
        ``indices``: int64 rows of the minibatch on the rows' device (one piece of ``ppo_minibatches``), or None for all rows in order.
        With ``normalize_advantage`` and more than one sample the minibatch advantages are normalised with SB3's own expression in torch
        and written back to their rows of a flat column the policy owns, which the library call then reads through the same indices (the
        C call never normalises).  ``.grad`` are views of two flat buffers the policy owns (allocated once, with the workspace), so
        ``clip_grad_norm_(policy.parameters(), 0.5); optimizer.step(); policy.update_weights()`` follow unchanged.  Returns the scalars
        ``loss``, ``policy_loss``, ``value_loss``, ``entropy_loss``, ``approx_kl``, ``clip_fraction`` as 0-dim tensors on the rows'
        device: nothing synchronises.  ``check``: a caller's own ``indices`` are validated with one ``torch.aminmax`` (the kernel does not
        range-check); pieces of ``ppo_minibatches`` for this row count skip it.  CUDA rows: rdv_ppo_loss_grad (the shipped 17-64-64 tanh actor and
        critic) or rdv_ppo_mlp_loss_grad (every other architecture the GPU forward serves) on the current stream; both differentiate
        the handles' weights as of stream order.  CPU rows or ``backend="torch"``: the same expressions through autograd over these
        modules, as for the one pair the library refuses (one net 64-64 tanh, the other not: ``ppo.hip_route``)."""
        from . import ppo
        return ppo.ppo_grad(self, buf, indices, clip_range, ent_coef, vf_coef, normalize_advantage, check)

    @torch.no_grad()
    def act(self, obs, deterministic=True, generator=None, out=None, env_id_offset=None):
        """SB3 ``predict``: the distribution mean (or a sample), clipped to the action Box.  HIP backend: the exploration noise of
        row i is keyed by (noise_seed, env_id_offset + i, call counter); ``env_id_offset`` defaults to ``noise_env_offset``."""
        hip = self.backend == "hip" or (self.backend == "auto" and obs.is_cuda and obs.dtype == torch.float32
                                        and obs.dim() == 2 and obs.shape[1] == 17)
        if hip:
            if generator is not None:
                self.noise_seed = int(generator.initial_seed())
            return self._act_hip(obs, deterministic, out, env_id_offset)
        a = self.mean(obs)
        if not deterministic:
            noise = torch.randn(a.shape, dtype=a.dtype, device=a.device, generator=generator)
            a = a + torch.exp(self.log_std) * noise
        return torch.clamp(a, -1.0, 1.0)

    def predict(self, observation, state=None, episode_start=None, deterministic=True):
        """SB3-compatible signature (monte_carlo.py:130-135) for NumPy observations."""
        dev = self.l1.weight.device
        obs = torch.as_tensor(np.asarray(observation), dtype=torch.float32, device=dev)
        return self.act(obs, deterministic=deterministic).cpu().numpy(), state


class PolicySet(_Members, _HipHandles):
    """P member policies of ONE architecture over one batch: member g owns the next ``group_sizes[g]`` rows, and one launch evaluates all
    members (include/rdv.h, "Policy sets"; csrc/rdv_policy_sets.h) — the network half of a sweep of P learners on one GPU, as a grouped
    ``RendezvousBatch`` is the environment half.  Row i of member g gets bit for bit what ``policies[g]`` alone computes for that row with
    the same noise seed, the same call counter and ``env_id_offset + start_g``.

    ``policies``: MlpPolicy objects with the same ``pi_arch``, ``vf_arch`` and ``activation`` (ValueError naming the first member that
    differs); they stay the source of truth for the weights (``set[g]``).  ``group_sizes``: positive, every one but the last a multiple
    of 256 rows, summing to ``num_rows`` when that is given — the rule and the messages of rdv_param_groups_check, checked on the host
    before any device is touched.  ``RendezvousBatch.act`` / ``rollout`` / ``collect`` take a set where they take an MlpPolicy; a set's
    ranges and the batch's parameter groups are independent.  One noise key for the whole set: ``noise_seed`` (default: member 0's) and
    the call counter ``_calls``.  CUDA float32 input goes to the set kernels; CPU input or ``backend="torch"`` loops the members'
    PyTorch modules over their slices."""

    _refresh_call = "rdv_policy_set_member_weights"

    def __init__(self, policies, group_sizes, num_rows=None, noise_seed=None, backend="auto"):
        self._init_members("PolicySet", MlpPolicy, ("pi_arch", "vf_arch", "activation"), policies, group_sizes, num_rows)
        self.backend = backend
        self.noise_seed = int(self.policies[0].noise_seed if noise_seed is None else noise_seed)
        self.noise_env_offset = 0
        self._calls = 0
        self._hip, self._hip_critic = {}, {}

    @property
    def has_critic(self):
        return all(p.has_critic for p in self.policies)

    @property
    def shipped_arch(self):
        return self.policies[0].shipped_arch

    # ------------------------------------------------------------------------------------------------ handles
    def _create_handle(self, prefix, idx):
        """rdv_policy_set_create / rdv_critic_set_create from the members' modules."""
        from . import _native as N
        arch = self.pi_arch if prefix == "l" else self.vf_arch
        host = [p._host_layers(prefix) for p in self.policies]        # kept alive until the call returns
        P, sizes, wpp, bpp, lsp = self._member_tables(host)
        spec = N.MlpSpec.make(arch, ACTIVATIONS[self.activation][0])
        N.check(N.lib().rdv_mlp_spec_check(C.byref(spec)))
        h = C.c_void_p()
        if prefix == "l":
            N.check(N.lib().rdv_policy_set_create(C.byref(spec), P, sizes, wpp, bpp, lsp, idx, C.byref(h)))
        else:
            N.check(N.lib().rdv_critic_set_create(C.byref(spec), P, sizes, wpp, bpp, idx, C.byref(h)))
        return h

    def _check_rows(self, n, what):
        if n != self.num_rows:
            raise ValueError(f"{what}: {n} rows, the policy set owns {self.num_rows}")

    # ------------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def act(self, obs, deterministic=True, generator=None, out=None, env_id_offset=None):
        """``MlpPolicy.act`` for the set: rows ``group_slices[g]`` of ``obs`` [n,17] through member g.  HIP: ONE launch
        (rdv_policy_act on the set handle), the noise of row i keyed by (noise_seed, env_id_offset + i, call counter).  CPU rows or
        ``backend="torch"``: the members' modules on their slices."""
        hip = self.backend == "hip" or (self.backend == "auto" and obs.is_cuda and obs.dtype == torch.float32
                                        and obs.dim() == 2 and obs.shape[1] == 17)
        self._check_rows(int(obs.shape[0]), "act")
        if hip:
            if generator is not None:
                self.noise_seed = int(generator.initial_seed())
            return self._act_hip(obs, deterministic, out, env_id_offset)
        parts = [p.act(obs[s], deterministic=deterministic, generator=generator) for p, s in zip(self.policies, self.group_slices)]
        res = torch.cat(parts, dim=0)
        if out is not None:
            out.copy_(res)
            return out
        return res

    def _value_torch(self, obs):
        """The members' critics (PyTorch modules) on observations [..., n, 17], each on its columns."""
        return torch.cat([p._value_torch(obs[..., s, :]) for p, s in zip(self.policies, self.group_slices)], dim=-1)

    @torch.no_grad()
    def value(self, obs, out=None):
        """The critics' values for observations [..., n, 17], n the set's rows: column i of every leading index through the member that
        owns row i.  HIP: one launch over all row blocks (rdv_policy_value on the critic set handle)."""
        if obs.dim() < 2 or obs.shape[-1] != 17:
            raise ValueError(f"value: expected [..., n, 17] observations, got {tuple(obs.shape)}")
        self._check_rows(int(obs.shape[-2]), "value")
        if self.backend != "torch" and obs.is_cuda and obs.dtype == torch.float32:
            return self._value_hip(obs, out)
        return self._value_torch(obs)

    @torch.no_grad()
    def advantages(self, ro, gamma=0.99, gae_lambda=0.95, out=None):
        """``MlpPolicy.advantages`` for the set: ``values``, ``last_value``, ``advantages`` and ``returns`` of the rows ``ro``, env i
        through the critic of the member that owns it; the same buffer reuse.  CUDA rows: rdv_rollout_advantages on the critic set
        handle (two critic launches over all members and the GAE kernel)."""
        if isinstance(ro.get("obs"), torch.Tensor) and ro["obs"].dim() == 3 and self.has_critic:
            self._check_rows(int(ro["obs"].shape[1]), "advantages")
        return _advantages(self, ro, gamma, gae_lambda, out)

    def ppo_grad(self, *args, **kwargs):
        """Not offered for a set: ``MlpPolicy.ppo_grad`` serves one actor and one critic (``ppo_grads`` serves all members at once)."""
        from . import ppo
        return ppo.ppo_grad(self, *args, **kwargs)

    def ppo_grads(self, buf, indices, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, check=True):
        """``MlpPolicy.ppo_grad`` for every member at once: the PPO loss of one minibatch per member and its gradients, written into
        ``.grad`` of the member modules' parameters (ppo.py; include/rdv.h "PPO minibatch gradients for policy sets").  ``buf``: the dict
        ``RendezvousBatch.collect(set, T)`` returns; ``buf["obs"]`` must be [T, N, 17] with N the set's rows.  ``indices``: a list of P
        int64 tensors of flat rows on the rows' device (one step of ``ppo_set_minibatches``), ``None`` for a member that sits this step
        out: its ``.grad`` is left as it was and its entry of the result is ``None``.  With ``check`` every member's indices that
        ``ppo_set_minibatches`` did not make for this set and T must be in range and lie in that member's env columns
        (``idx % N`` in its slice; IndexError), which also keeps the members' rows disjoint.  One clip_range / ent_coef / vf_coef for
        all members.  CUDA rows, the shipped 17-64-64 tanh architecture, ``backend != "torch"``: the indices are concatenated into a
        buffer the set owns (the counts are the tensors' sizes: nothing is read from the device), the advantages are normalised per
        member with SB3's expression on its own minibatch — the expression of ``ppo_grad``, hence its bits — into one advantage column
        the set owns, and ONE rdv_ppo_set_loss_grad runs on the current stream.  The gradients land in two buffers [P,5708] and
        [P,5377] the set owns; member g's ``.grad`` tensors are views of row g, so per-member ``clip_grad_norm_``, one optimiser over
        all members' parameters and ``update_weights()`` follow unchanged.  Every member's gradients and scalars are bit for bit those
        of its own ``MlpPolicy.ppo_grad`` on the same buffer and indices.  A set of another architecture the forward kernels serve
        (``ppo.hip_set_route`` answers "mlp": 1..4 hidden layers of 16 / 32 / 64, tanh, ReLU or sigmoid, at most 64 members) takes
        the same path through ONE rdv_ppo_mlp_set_loss_grad, its buffers [P,Ga] and [P,Gc] of the architecture's gradient lengths,
        with the same equality.  CPU rows, ``backend="torch"``, an unserved width or exactly one net of the shipped shape:
        ``ppo.ppo_grad`` member by member.  Returns a list of P dicts of 0-dim tensors (the scalars of ``ppo_grad``)."""
        from . import ppo
        return ppo.ppo_set_grads(self, buf, indices, clip_range, ent_coef, vf_coef, normalize_advantage, check)

    def adam_step(self, stepped=None, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5):
        """What follows ``ppo_grads`` in a learner's step, for every member at once: SB3's ``clip_grad_norm_(policy.parameters(),
        max_grad_norm)`` per member (actor and critic under ONE norm), ``torch.optim.Adam(eps=eps)`` and the refresh of the members'
        forward weights (ppo.py; include/rdv.h "Gradient clip, Adam and weight repack for policy sets").  ``stepped``: the list
        ``ppo_grads`` returned; a member whose entry is ``None`` sits out (its weights, moments and step count stay).  ``None``: all
        members step.  One lr / betas / eps / max_grad_norm for all members; no weight decay, no AMSGrad.

        After a ``ppo_grads`` that ran rdv_ppo_set_loss_grad (CUDA rows, the shipped 17-64-64 tanh architecture, at most 64 members,
        ``backend != "torch"``) this is ONE call of rdv_ppo_set_adam_step on the current stream of that device: no allocation past the
        first use, no synchronisation, no host copy, legal inside a stream capture (each replay takes the next step).  On first use the
        set allocates the fp32 master weights [P,5708] / [P,5377], the moments and the step counters on that device, fills the weights
        from the member modules and re-points the members' parameters at views of row g (the modules move to that device), as their
        ``.grad`` are views of the gradient buffers.  So ``state_dict()`` and checkpoints see the stepped weights with no copy, and NO
        ``update_weights()`` is needed: the call itself rewrites the members' forward blocks on the device — the bytes
        ``update_weights()`` would pack, but for the six ``exp(log_std)`` floats of an actor block: the double-precision exp rounded
        to float on both sides, through two libraries' exp — promised within 1 ulp, and equal but for a double result next to a float
        rounding boundary; deterministic actions and values do not read them, sampled actions and gradients do.  A member
        whose gradient norm is not finite is skipped whole and flagged.  ``update_weights(member=, weights=)`` writes through the views
        and keeps the moments: ``reset_optimizer`` zeroes them.

        A set of another architecture the forward kernels serve, after a ``ppo_grads`` that ran rdv_ppo_mlp_set_loss_grad, takes ONE
        rdv_ppo_mlp_set_adam_step under the same contract: master weights, moments and views of the architecture's lengths [P,Ga] /
        [P,Gc], the forward blocks the bytes ``update_weights()`` would pack but for the six ``exp(log_std)`` floats.

        CPU rows, ``backend="torch"``, an unserved width or exactly one net of the shipped shape: per-member ``clip_grad_norm_`` and one ``torch.optim.Adam`` the set owns
        over all members' parameters; the moments are then PyTorch's, a member with a non-finite norm is left out of that step, and
        ``update_weights()`` follows as before.  Which of the two runs is decided by the LAST ``ppo_grads``: behind one that went member
        by member, a set that has stepped on the device takes the PyTorch step too (on its parameters, the views of the master weights);
        the device moments and step counters are left as they are, and a later device ``ppo_grads`` + ``adam_step`` continues from them.

        Returns a dict of [P] tensors on the rows' device: ``total_norm``, ``clip_coef``, ``skipped`` (1.0: the member's norm was not
        finite); the entries of a member that sat out are those of its last step (zero before the first)."""
        from . import ppo
        return ppo.set_adam_step(self, stepped, lr, betas, eps, max_grad_norm)

    def reset_optimizer(self, member=None):
        """Zero the Adam moments and the step counter of one member (``member`` = its index) or of all (None), on the device state and
        in the fallback's optimiser alike; the weights are not touched.  For a member whose weights were replaced through
        ``update_weights(member=, weights=)`` and should start its optimiser afresh."""
        from . import ppo
        return ppo.set_reset_optimizer(self, member)
