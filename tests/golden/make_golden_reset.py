#!/usr/bin/env python3
"""
Golden fixture for reset(): the uniform -> initial-state map of the UNMODIFIED `RendezvousEnv.reset()` (rendezvous_env.py:223-270),
recorded for the counter-based uniforms the project draws (Philox4x32-10 keyed by seed / global env id / episode, pinned by the
Random123 known-answer test), at parameter sets whose nominal attitudes are rotated and non-unit — where the factor order and
cross-term signs of quat_product, the normalisation of the nominal and the lvlh2chaser / lvlh2target rotations do not cancel.

    python tests/golden/make_golden_reset.py      # seconds; needs /root/reference

While the reference's own reset() runs, `np.random.uniform` is a feeder that hands out `low + (high - low) * u` for the next of the
row's 24 uniforms and counts them; the reference's files are not touched.  Written: tests/golden/reset_reference.npz
  kwargs[S]            constructor kwargs of the S = 7 parameter sets, JSON (as params_reference.npz)
  seed, env_ids[N], episodes[E]
  uniforms[E,N,24]     what oracle.philox_uniforms(seed, env id, episode) returned (the same for every set)
  state[S,E,N,20] f64, obs[S,E,N,17] f32, collided[S,E,N], success[S,E,N]
  flags_robust[S,E,N]  the reference's flag decisions of the row all have a margin (see robust_flags): only such rows are compared
                       with a kernel that stores its state in float32
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from make_golden import OUT, install_stubs, state20   # noqa: E402

SEED = 0x9E3779B97F4A7C15                 # high word 0x9E3779B9: the key's second word is not zero
N_ENVS = 160                              # 2 1/2 wavefronts
ENV_ID0 = 2 ** 32 - 80                    # the ids cross 2^32: both counter words change inside the batch
EPISODES = (0, 1, 2)
TINY_SWITCH = 2 * np.sqrt(0.0078125)      # the attitude range at which the kernels change series: (range / 2)^2 = 2^-7
MARGIN = 1e-5


def _unit(q):
    q = np.asarray(q, float)
    return q / np.linalg.norm(q)


def _rotate(q, v):
    """R(q) v for a unit quaternion (scalar first), written out here: the port-side nominal of set (c) is built with it."""
    w, x, y, z = q
    R = np.array([[2 * (w * w + x * x) - 1, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 2 * (w * w + y * y) - 1, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 2 * (w * w + z * z) - 1]])
    return R @ np.asarray(v, float)


def _port_start():
    """(c): the chaser at the docking port of a rotated, spinning target, pointing at it, moving and turning with it — so that the
    sampled deviations straddle every limit of check_success, and the corridor's cone of check_collision."""
    qt = _unit([0.8, 0.3, -0.4, 0.33])
    wt = np.array([0.012, -0.02, 0.016])                     # LVLH (:258 converts to the target's frame)
    rc = _rotate(qt, [0.0, -2.0, 0.0])                       # target2lvlh(rd)
    vc = np.cross(wt, rc)                                    # the port's velocity (:461)
    # a chaser attitude with R(qc) [0,1,0] = -rc/|rc|: the shortest rotation from +y to that direction
    a, b = np.array([0.0, 1.0, 0.0]), -rc / np.linalg.norm(rc)
    # (after a roll of 0.9 rad about the capture axis itself, which leaves the axis where it is and fills all four components)
    s1, v1 = np.cos(0.45), np.sin(0.45) * a
    q0 = _unit(np.append(1.0 + a @ b, np.cross(a, b)))
    qc = np.append(q0[0] * s1 - q0[1:] @ v1, q0[0] * v1 + s1 * q0[1:] + np.cross(q0[1:], v1))
    return dict(rc0=rc.tolist(), vc0=vc.tolist(), qc0=(1.3 * qc).tolist(), wc0=wt.tolist(), qt0=(0.7 * qt).tolist(), wt0=wt.tolist(),
                rc0_range=1.2, vc0_range=0.12, qc0_range=float(np.radians(6)), wc0_range=float(np.radians(0.7)),
                qt0_range=0.3, wt0_range=float(np.radians(0.7)))


ROTATED = dict(qc0=[1.53, 0.17, -0.34, 0.51], qt0=[0.6, -1.4, 0.8, 1.0], vc0=[0.02, -0.03, 0.01], wc0=[0.004, -0.002, 0.003],
               wt0=[0.01, -0.02, 0.03])
SETS = [
    ("a_default", {}),
    ("b_rotated", dict(ROTATED, qt0_range=float(np.pi))),
    ("c_port", _port_start()),
    ("d_zero_ranges", dict(ROTATED, rc0=[0.5, -9.0, -0.25], rc0_range=0.0, vc0_range=0.0, qc0_range=0.0, wc0_range=0.0, qt0_range=0.0,
                           wt0_range=0.0)),
    ("e_switch", dict(ROTATED, qc0_range=float(TINY_SWITCH * (1 - 1e-9)), qt0_range=float(TINY_SWITCH * (1 + 1e-9)))),
    ("f_switch_reversed", dict(ROTATED, qc0_range=float(TINY_SWITCH * (1 + 1e-9)), qt0_range=float(2 * np.sqrt(0.0078125)))),
    ("g_wide", dict(ROTATED, rc0=[3.0, -9.0, 2.0], rc0_range=6.0, vc0_range=1.5, qc0_range=float(np.pi), wc0_range=float(np.radians(4)),
                    qt0_range=float(np.pi), wt0_range=float(np.radians(8)), h=400e3, dt=0.5, t_max=90)),
]


class Feeder:
    """Stands in for np.random.uniform while one reset() runs: the row's uniforms, in the order they are asked for."""

    def __init__(self):
        self.u, self.k = None, 0

    def load(self, u):
        self.u, self.k = u, 0

    def __call__(self, low=0.0, high=1.0, size=None):
        n = 1 if size is None else int(np.prod(size))
        u = self.u[self.k:self.k + n]
        assert len(u) == n, "reset() asked for more than 24 uniforms"
        self.k += n
        out = low + (high - low) * u
        return float(out[0]) if size is None else out.reshape(size)


def _decisive_k(limit, strict):
    """Largest k in [-1e5, 1e5] with acos(k/1e5) > limit (strict) or >= limit: general.py:179 rounds the cosine to k/1e5."""
    k = np.arange(-100000, 100001)
    ang = np.arccos(k / 1e5)
    hit = k[ang > limit] if strict else k[ang >= limit]
    return int(hit.max()) if hit.size else -100001


def _cos_margins(v1, v2, k_decisive):
    """For angle_between_vectors(v1, v2) compared with a limit whose last k on the far side is k_decisive: is 1e5 cos away from every
    rounding tie by more than MARGIN of the rounding unit, away from the one tie that decides the comparison (k_decisive + 0.5) by more
    than MARGIN of the cosine (1 unit of k at |cos| = 1: float32 storage moves 1e5 cos by ~0.1), and is the rounded cosine itself more
    than MARGIN (relative) away from the limit's cosine."""
    x = 1e5 * (np.dot(v1, v2) / (np.linalg.norm(v1) * np.linalg.norm(v2)))
    tie = abs(x - np.floor(x) - 0.5) > MARGIN
    decisive = abs(x - (k_decisive + 0.5)) > MARGIN * 1e5 * max(abs(k_decisive + 0.5) / 1e5, MARGIN)
    return tie and decisive


def robust_flags(env, kc_coll, ka_succ):
    """True where every comparison behind `collided` and `success` (:388-422) has a relative margin above MARGIN in the reference's own
    numbers: |rc| against koz_radius; the corridor cosine against its rounding ties and the corridor's threshold; the four errors against
    their limits (the attitude error through its rounded cosine as well).  A kernel that keeps its state in float32 perturbs these
    quantities by ~1e-7 relative, two orders below the margin; a row without the margin may legitimately decide the other way."""
    r = np.linalg.norm(env.rc)
    ok = abs(r - env.koz_radius) > MARGIN * env.koz_radius
    axis = env.target2lvlh(env.corridor_axis)
    ok = ok and _cos_margins(env.rc, axis, kc_coll)
    cos_limit = np.cos(env.corridor_half_angle)
    ok = ok and abs(round(np.dot(env.rc, axis) / (r * np.linalg.norm(axis)), 5) - cos_limit) > MARGIN * abs(cos_limit)
    err = env.get_errors()
    lim = np.array([env.max_rd_error, env.max_vd_error, env.max_qd_error, env.max_wd_error])
    ok = ok and bool(np.all(np.abs(err - lim) > MARGIN * lim))
    ok = ok and _cos_margins(-env.rc, env.chaser2lvlh(env.capture_axis), ka_succ)
    return bool(ok)


def main():
    install_stubs()
    import oracle
    from rendezvous_env import RendezvousEnv
    ids = ENV_ID0 + np.arange(N_ENVS, dtype=np.uint64)
    uniforms = np.array([[oracle.philox_uniforms(SEED, int(i), e) for i in ids] for e in EPISODES])      # [E, N, 24]
    S, E, N = len(SETS), len(EPISODES), N_ENVS
    state = np.zeros((S, E, N, 20)); obs = np.zeros((S, E, N, 17), np.float32)
    collided = np.zeros((S, E, N), np.uint8); success = np.zeros((S, E, N), np.uint8); robust = np.zeros((S, E, N), bool)
    feeder = Feeder()
    genuine = np.random.uniform
    np.random.uniform = feeder
    try:
        for s, (name, kw) in enumerate(SETS):
            env = RendezvousEnv(quiet=True, **{k: (np.array(v, dtype=float) if isinstance(v, list) else v) for k, v in kw.items()})
            kc_coll = _decisive_k(env.corridor_half_angle, True)         # collided  <=> k <= kc_coll            (:401, angle > half angle)
            ka_succ = _decisive_k(env.max_qd_error, True)                # att error <= limit <=> k > ka_succ    (:417)
            for e in range(E):
                for i in range(N):
                    feeder.load(uniforms[e, i])
                    o = env.reset()
                    assert feeder.k == 24, f"reset() consumed {feeder.k} uniforms, not 24"
                    state[s, e, i] = state20(env); obs[s, e, i] = o
                    collided[s, e, i] = bool(env.collided); success[s, e, i] = int(env.success)
                    robust[s, e, i] = robust_flags(env, kc_coll, ka_succ)
            share = robust[s].mean()
            print(f"{name}: collided {int(collided[s].sum())}, success {int(success[s].sum())}, robust {share:.3f}")
            assert share >= 0.9, f"{name}: only {share:.3f} of the rows have robust flags; choose other nominals"
    finally:
        np.random.uniform = genuine
    c = [n for n, _ in SETS].index("c_port")
    assert collided[c].sum() >= 10 and success[c].sum() >= 10, (int(collided[c].sum()), int(success[c].sum()))
    assert np.isfinite(state).all() and np.isfinite(obs).all()
    path = os.path.join(OUT, "reset_reference.npz")
    np.savez_compressed(path, kwargs=np.array([json.dumps(kw) for _, kw in SETS]), names=np.array([n for n, _ in SETS]),
                        seed=np.uint64(SEED), env_ids=ids, episodes=np.array(EPISODES, np.uint32), uniforms=uniforms, state=state, obs=obs,
                        collided=collided, success=success, flags_robust=robust)
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print(f"reset_reference.npz: {S} sets x {E} episodes x {N} envs, {size} bytes")


if __name__ == "__main__":
    main()
