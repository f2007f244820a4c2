#!/usr/bin/env python3
"""
Golden fixture for the comparisons the product turns into host-derived limits (thresholds_reference.npz): the time limit
`t = round(t + dt, 3); t >= t_max` (rendezvous_env.py:193, :368), the norm limits `np.linalg.norm(x) <= limit` / `< limit`
(:416, :348, :397) at other values than the defaults, and the angle limits `arccos(round(cos, 5)) > / <= / < theta` (general.py:179,
rendezvous_env.py:370, :401, :417, :350).  Everything is asked of the UNMODIFIED reference env (same inert import stubs as
make_golden.py): get_errors() (:451), check_collision() (:388), check_success() (:406), dist_from_koz() (:510) and step() (:160) with
a zero action.  Parameter sets are given the way monte_carlo.py:107-112 gives state: as attribute assignments on the env (dt and
t_max as constructor arguments, because the constructor derives the bubble rate from dt).

Three sections (arrays `time_*`, `norm_*`, `angle_*`); every row holds its parameter overrides (an index into `*_sets_json`), its
state and the reference's outputs.

  time   one row per (dt, t_max): a bit-exact fixed point of a zero-action step (chaser at rest on the V-bar, identity attitudes,
         target at rest), stepped until done; env.t after every step, the step on which it is done, the reason ("time" in every row).
  norm   the constructions of make_golden_boundary.py (one non-zero component, value on the limit and 1-2 ulp either side; scaled
         generic directions) at limits whose squares are not representable, a limit whose square underflows and one whose square
         overflows.  The position rows are V-bar fixed points: the port is moved to rd = (0, -2^e, 0), 2^e the power of two above the
         limit (1.5 x the limit where that is a power of two itself), and the chaser sits between port and target, so that
         rc_y - rd_y IS the placed value (the subtraction is exact).
  angle  states whose cosine sits in the middle of the gap between two entries of the 5-decimal grid, 1e5*cos = k + 0.5 -+ 1e-3, for
         the k next to each limit; each a fixed point.  The generator asserts that the reference reads k and k + 1.

Rows flagged `fixed` are fixed points of a zero-action step and also carry three reference steps (state, aux, reward, done, reason,
diagnostics); the other rows (a moving or spinning chaser) carry the diagnostics of the placed state only: one step moves their
norms off the limit by far more than an ulp, and by another amount under scipy's RK45 than under the closed form.

`acos_sides_agree[i]`: np.arccos and math.acos (libm) put every entry of the 200,001-entry table k/1e5 on the same side of
`acos_limits[i]` under >, >=, < and <=.  The reference's own answer at a tie depends on its NumPy build.

    python tests/golden/make_golden_thresholds.py      # seconds; needs /root/reference (build container only)
"""
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, aux6, diag8, install_stubs, state20   # noqa: E402
from make_golden_boundary import around                            # noqa: E402

STEPS = 3                       # reference steps recorded for a fixed-point row
DEG = [5, 15, 25, 30, 35, 45, 60, 90]


def base_state(y):
    s = np.zeros(20)
    s[1] = y; s[6] = 1.0; s[13] = 1.0
    return s


def assign(env, s, overrides):
    for k, v in overrides.items():
        setattr(env, k, np.array(v, dtype=np.float64) if isinstance(v, list) else v)
    env.rc, env.vc, env.qc = s[0:3].copy(), s[3:6].copy(), s[6:10].copy()
    env.wc, env.qt, env.wt = s[10:13].copy(), s[13:17].copy(), s[17:20].copy()


def reason_of(env, obs):
    conds = [not env.observation_space.contains(obs), env.t >= env.t_max,
             np.linalg.norm(env.rc) > env.bubble_radius, env.get_attitude_error() > env.max_attitude_error]
    return conds.index(True) + 1


def fresh_env(RendezvousEnv, **ctor):
    env = RendezvousEnv(quiet=True, **ctor)
    np.random.seed(0)
    env.reset()
    assert not env.collided and env.success == 0 and env.t == 0
    return env


# ---------------------------------------------------------------------------------------------------------------- (a) time
TIME_CASES = [
    (0.25, [7.3, 10]), (0.5, [7.3, 9.999, 10, 10.001]), (1.0, [60, 120]), (1, [60]), (2.0, [61, 120]), (4.0, [119.999, 120]),
    (0.1, [9.999, 10, 10.001]), (0.05, [4.975, 5]), (0.01, [2.999, 3, 3.001]), (0.001, [0.2995, 0.3]), (0.125, [9.9, 10]),
    (0.3, [20, 20.1]), (0.7, [20, 21]), (1.1, [60, 60.5]), (5.0, [120, 121]), (20.0, [120, 400]),
    (1 / 3, [60]), (0.0625, [20]), (0.15625, [5]), (0.0125, [5]), (0.0025, [0.8]), (0.0015, [0.5]), (0.1234, [45]), (1 / 7, [50]),
]


def k_time_rule(dt, t_max):
    """The product's closed form (csrc/rdv_hip.hip, derive_params): first k with rint(k*dt*1e3)/1e3 >= t_max.  Printed beside the
    reference's own step, never stored."""
    k = 0
    while np.rint(k * dt * 1e3) / 1e3 < t_max:
        k += 1
    return k


def time_section(RendezvousEnv):
    s = base_state(-2.25)       # inside the sphere and the corridor, below bubble_min: neither bubble nor attitude can end the episode
    rows = [(dt, t_max) for dt, ts in TIME_CASES for t_max in ts]
    depth = 0
    rec = dict(dt=[], dt_is_int=[], t_max=[], t=[], done_step=[], reason=[], is_ms=[])
    for dt, t_max in rows:
        env = fresh_env(RendezvousEnv, dt=dt, t_max=t_max)
        assign(env, s, {})
        ts = []
        for k in range(1, 1000):
            obs, _, done, _ = env.step(np.zeros(6, np.float32))
            assert (state20(env) == s).all(), "the time rows must be fixed points"
            ts.append(float(env.t))
            if done:
                break
        reason = reason_of(env, obs)
        assert done and reason == 2, (dt, t_max, reason)
        is_ms = float(dt) == np.rint(float(dt) * 1e3) / 1e3
        rule = k_time_rule(float(dt), float(t_max))
        closed = all(t == np.rint(j * float(dt) * 1e3) / 1e3 for j, t in enumerate(ts, 1))
        print(f"time dt={dt!r} t_max={t_max!r}: done on step {k} (k_time rule {rule}), multiple of 1 ms: {is_ms}, "
              f"t equals rint(k*dt*1e3)/1e3 on every step: {closed}")
        assert not is_ms or (rule == k and closed), "a dt that is a multiple of 1 ms must follow the closed form"
        rec["dt"].append(float(dt)); rec["dt_is_int"].append(isinstance(dt, int)); rec["t_max"].append(float(t_max))
        rec["t"].append(ts); rec["done_step"].append(k); rec["reason"].append(reason); rec["is_ms"].append(is_ms)
        depth = max(depth, k)
    t = np.full((len(rows), depth), np.nan)
    for i, ts in enumerate(rec["t"]):
        t[i, :len(ts)] = ts
    return dict(time_dt=np.array(rec["dt"]), time_dt_is_int=np.array(rec["dt_is_int"], np.uint8), time_t_max=np.array(rec["t_max"]),
                time_dt_is_ms=np.array(rec["is_ms"], np.uint8), time_t=t, time_done_step=np.array(rec["done_step"], np.int32),
                time_reason=np.array(rec["reason"], np.uint8), time_state=s)


# ---------------------------------------------------------------------------------------------------------------- (b) norms
LIMITS = [0.1, 0.3, 1 / 3, 1e-3, 2.0, float(np.radians(1))]
KOZ = [2, 2.5, 5, 7.5, 10, 0.1 + 0.2]
TINY, HUGE = 1e-160, 1e200


def port_for(x):
    """|rd_y| for a position limit x: the power of two above x (1.5 x where x is one itself), so that port - x' lies in no coarser
    binade than x' for x' = x and its neighbours, and rc_y = -(port - x') and rc_y - rd_y = x' are both exact."""
    e = 2.0 ** math.ceil(math.log2(x))
    return 1.5 * x if e == x else e


def norm_cases():
    """[(overrides, [(kind, value, state, fixed)])]"""
    rng = np.random.default_rng(11)
    out = []

    def directions(limit, lo, centre):
        rows = []
        for _ in range(6):
            u = rng.normal(size=3); u /= np.linalg.norm(u)
            for x in around(limit, 1):
                s = base_state(-2.25)
                s[lo:lo + 3] = centre + u * x
                rows.append(({0: "pos3", 3: "vel3", 10: "rot3"}[lo], x, s, False))
        return rows

    for limit in LIMITS:
        port = port_for(limit)                                        # rd = (0, -port, 0): rdn - max_rd_error > 0, rdn < koz_radius
        rows = []
        for x in around(limit):                                       # chaser between port and target: rc_y - rd_y = x exactly
            s = base_state(-port + x)
            assert s[1] < 0 and s[1] - (-port) == x
            rows.append(("pos", x, s, True))
        rows += directions(limit, 0, np.array([0.0, -port, 0.0]))
        out.append((dict(max_rd_error=limit, rd=[0.0, -port, 0.0]), rows))
    # x*x underflows to a subnormal or to zero.  A port 1e-160 m from the target leaves no direction to measure an attitude in, so
    # the port stays where it is and the chaser sits beside it, off the V-bar (rc - rd = (x, 0, 0) exactly; not a fixed point)
    rows = []
    for x in around(TINY) + [1e-170, 0.5e-160, 2e-160, 3e-160]:
        s = base_state(-2.0); s[0] = x
        rows.append(("pos-x", x, s, False))
    out.append((dict(max_rd_error=TINY), rows))
    for name, kind, lo in (("max_vd_error", "vel", 3), ("max_wd_error", "rot", 10)):
        for limit in LIMITS + [TINY, HUGE]:
            rows = []
            for x in around(limit):
                s = base_state(-2.25); s[lo] = x
                rows.append((kind, x, s, False))
            if limit == TINY:
                for x in (1e-170, 0.5e-160, 2e-160, 3e-160):
                    s = base_state(-2.25); s[lo] = x
                    rows.append((kind, x, s, False))
            elif limit == HUGE:                                        # x*x overflows from 1.34e154 on: every norm below is <= limit
                for x in (1e150, 1.3e154, 1.35e154, 1e155):
                    s = base_state(-2.25); s[lo] = x
                    rows.append((kind, x, s, False))
            else:
                rows += directions(limit, lo, np.zeros(3))
            out.append(({name: limit}, rows))
    q90 = [np.cos(np.pi / 4), 0.0, 0.0, np.sin(np.pi / 4)]            # target turned 90 deg about z: the corridor axis leaves the V-bar
    for r in KOZ + [HUGE]:
        ov = dict(koz_radius=r)
        if r <= 2:                                                    # the port must lie inside the sphere (:155) and keep :156
            ov.update(rd=[0.0, -r / 2, 0.0], max_rd_error=r / 4)
        rows = []
        xs = around(r) + ([1e150, 1.3e154, 1.35e154] if r == HUGE else [])
        for x in xs:                                                  # |rc| = x, 90 deg off the corridor axis: collision iff inside
            s = base_state(0.0); s[0] = x
            rows.append(("koz", x, s, False))
            if x <= 10:                                               # the same on the V-bar (a fixed point), inside the bubble
                s = base_state(-x); s[13:17] = q90
                rows.append(("koz-vbar", x, s, True))
        out.append((ov, rows))
    return out


# ---------------------------------------------------------------------------------------------------------------- (c) angles
def turned(phi):
    return [np.cos(phi / 2), 0.0, 0.0, np.sin(phi / 2)]


def angle_cases(default_att, default_qd, default_corr):
    """[(overrides, limit, [(kind, k_read, state)])]: every construction is a fixed point.  kinds: att-done (outside the sphere: the
    episode ends iff att > max_attitude_error), att-succ (at the port, zero position error: success iff att <= max_qd_error),
    att-bonus (in the corridor, position error below its limit: the second bonus iff att < max_qd_error), corridor (3 m on the
    V-bar, target turned: collision iff angle > corridor_half_angle)."""
    def rows_for(kind, theta):
        k0 = int(np.rint(1e5 * np.cos(theta)))
        places = []
        for k in (k0 - 2, k0 - 1, k0, k0 + 1):
            for side, k_read in ((-1e-3, k), (+1e-3, k + 1)):
                places.append((np.arccos((k + 0.5 + side) / 1e5), k_read))
        if theta == np.pi / 2:
            places.append((np.pi / 2, 0))                              # exactly perpendicular: the tie that is exact in every acos
        out = []
        for phi, k_read in places:
            if kind == "corridor":
                s = base_state(-3.0); s[13:17] = turned(phi)
            else:
                s = base_state({"att-done": -8.0, "att-succ": -2.0, "att-bonus": -2.25}[kind]); s[6:10] = turned(phi)
            out.append((kind, k_read, s))
        return out

    sets = [({}, np.nan, rows_for("att-done", default_att) + rows_for("att-succ", default_qd) + rows_for("att-bonus", default_qd)
             + rows_for("corridor", default_corr))]
    for deg in DEG:
        theta = np.pi / 2 if deg == 90 else float(np.radians(deg))
        ov = dict(max_attitude_error=theta, max_qd_error=theta, corridor_half_angle=theta)
        sets.append((ov, theta, [r for kind in ("att-done", "att-succ", "att-bonus", "corridor") for r in rows_for(kind, theta)]))
    return sets


def acos_tables():
    ks = np.arange(-100000, 100001)
    ref = np.array([float(np.arccos(np.float64(k) / 1e5)) for k in ks])     # scalar calls, as general.py:179 makes them
    libm = np.array([math.acos(float(k) / 1e5) for k in ks])
    return ref, libm


def sides_agree(theta, ref, libm):
    return bool(((ref > theta) == (libm > theta)).all() and ((ref >= theta) == (libm >= theta)).all())   # <, <= are their negations


# ---------------------------------------------------------------------------------------------------------------- recording
def record_rows(RendezvousEnv, prefix, sets):
    """sets: [(overrides, rows)], rows (kind, value, state, fixed)."""
    kinds, values, states, set_of, fixed, diag = [], [], [], [], [], []
    st, aux, rew, done, reason, sdiag = [], [], [], [], [], []
    for j, (ov, rows) in enumerate(sets):
        for kind, value, s, fx in rows:
            env = fresh_env(RendezvousEnv)
            assign(env, s, ov)
            kinds.append(kind); values.append(value); states.append(s); set_of.append(j); fixed.append(fx)
            diag.append(diag8(env))
            r = dict(st=np.full((STEPS, 20), np.nan), aux=np.full((STEPS, 6), np.nan), rew=np.full(STEPS, np.nan),
                     done=np.zeros(STEPS, np.uint8), reason=np.zeros(STEPS, np.uint8), sdiag=np.full((STEPS, 8), np.nan))
            if fx:
                for t in range(STEPS):
                    obs, rw, dn, _ = env.step(np.zeros(6, np.float32))
                    r["st"][t], r["aux"][t], r["rew"][t], r["done"][t], r["sdiag"][t] = state20(env), aux6(env), float(rw), dn, diag8(env)
                    if dn:
                        r["reason"][t] = reason_of(env, obs)
                assert (r["st"][1:] == r["st"][0]).all(), (prefix, kind, value, "not a fixed point of the reference's step")
                assert np.abs(r["st"][0] - s).max() <= 2.3e-16, (prefix, kind, value)      # the :574 normalisation may move a turned quaternion by an ulp
            st.append(r["st"]); aux.append(r["aux"]); rew.append(r["rew"]); done.append(r["done"]); reason.append(r["reason"]); sdiag.append(r["sdiag"])
    p = prefix + "_"
    return {p + "sets_json": np.array([json.dumps(ov) for ov, _ in sets]), p + "set": np.array(set_of, np.int32),
            p + "kind": np.array(kinds), p + "value": np.array(values, np.float64), p + "state": np.stack(states),
            p + "fixed": np.array(fixed, np.uint8), p + "diag": np.stack(diag), p + "step_state": np.stack(st),
            p + "step_aux": np.stack(aux), p + "step_reward": np.stack(rew), p + "step_done": np.stack(done),
            p + "step_reason": np.stack(reason), p + "step_diag": np.stack(sdiag)}


def main():
    install_stubs()
    from rendezvous_env import RendezvousEnv
    from utils.general import angle_between_vectors
    out = time_section(RendezvousEnv)

    out.update(record_rows(RendezvousEnv, "norm", norm_cases()))

    env = fresh_env(RendezvousEnv)
    sets = angle_cases(env.max_attitude_error, env.max_qd_error, env.corridor_half_angle)
    for ov, _, rows in sets:                       # the two sides of every gap really read k and k + 1 on the reference
        for kind, k_read, s in rows:
            assign(env, s, {})
            got = (angle_between_vectors(env.rc, env.target2lvlh(env.corridor_axis)) if kind == "corridor" else env.get_attitude_error())
            assert got == np.arccos(k_read / 1e5), (kind, k_read, got)
    out.update(record_rows(RendezvousEnv, "angle", [(ov, [(kind, k, s, True) for kind, k, s in rows]) for ov, _, rows in sets]))
    ref, libm = acos_tables()
    limits = sorted({float(v) for ov, _, _ in sets for v in ov.values()} | {env.max_attitude_error, env.max_qd_error, env.corridor_half_angle})
    out["acos_limits"] = np.array(limits)
    out["acos_sides_agree"] = np.array([sides_agree(th, ref, libm) for th in limits], np.uint8)
    out["acos_table_diff_count"] = np.array(int((ref != libm).sum()))
    out["acos_table_max_ulp"] = np.array(float(np.max(np.abs(ref - libm) / np.spacing(np.maximum(ref, libm)))))
    out["study_limits"] = np.array([float(np.radians(d)) for d in (15, 25, 30, 35, 45)] + [float(np.radians(5))])
    # angle sets whose limits the two acos agree on (the default set's three limits are the first entries of study_limits)
    agree = {th: a for th, a in zip(limits, out["acos_sides_agree"])}
    out["angle_set_sides_agree"] = np.array([all(agree[float(v)] for v in ov.values()) if ov else
                                             all(agree[float(x)] for x in (env.max_attitude_error, env.max_qd_error, env.corridor_half_angle))
                                             for ov, _, _ in sets], np.uint8)
    path = os.path.join(OUT, "thresholds_reference.npz")
    np.savez_compressed(path, **out)
    print("acos table: np.arccos != math.acos in", int(out["acos_table_diff_count"]), "of", len(ref), "entries, max",
          float(out["acos_table_max_ulp"]), "ulp; sides agree:", {round(np.degrees(th), 6): bool(a) for th, a in agree.items()})
    for p in ("norm", "angle"):
        d = out[p + "_diag"]
        print(f"{p}: {len(d)} rows in {len(out[p + '_sets_json'])} parameter sets, {int(out[p + '_fixed'].sum())} fixed points; "
              f"success flags {int(d[:, 5].sum())}, collision flags {int(d[:, 4].sum())}, done rows {int(out[p + '_step_done'][:, 0].sum())}")
    print(len(out["time_dt"]), "time rows, deepest", out["time_t"].shape[1], "steps ->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
