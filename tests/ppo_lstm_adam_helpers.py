"""
What the tests of rdv_lstm_ppo_set_adam_step share (include/rdv.h, "Gradient clip, Adam and weight repack for recurrent policy sets";
csrc/rdv_ppo_lstm_adam.h): the flat layout of a recurrent net's parameters (rdv_lstm_ppo_grad_floats: w_ih, w_hh, b_ih, b_hh, the trunk's
layers, log_std), a NumPy restatement of the host packer of a recurrent handle's block [trunk block | cell block]
(pack_lstm_weights, csrc/rdv_policy_lstm.h), the four corners of the cell's ONE shift, and the comparison of two blocks as the header
states it.  The references of the step itself are tests/ppo_adam_reference.py's (coef32, step32, step64, bound: counted per entry, they
carry over to rows of any length); members and rollouts are tests/ppo_lstm_set_helpers.py's.  Runs on the CPU.
"""
import numpy as np

import policy_lstm_reference as L
import policy_reference as R
import ppo_adam_reference as A

f32 = np.float32
IN, OUT = 17, 6
MLP_REC, MLP_REC_STRIDE, MLP_STD, MLP_HDR = 8, 8, 48, 128          # kMlpRec, kMlpRecStride, kMlpStd, kMlpHdr of csrc/rdv_policy_mlp.h
CELL_HDR, X_SHIFT, FRAG_FLOATS = 4, 10, 256                        # kLstmCellHdr, kPolXShift, kPolFragBytes / 4
ACT_CODES = {"tanh": 0, "relu": 1, "sigmoid": 2}
CORNERS = ("hh_dominates", "ih_dominates", "negative_shift", "zero_lstm")


# ------------------------------------------------------------------------------------------------------------ layouts
def flat(net, actor):
    """A policy_lstm_reference network in the flat layout of rdv_lstm_ppo_grad_floats."""
    parts = [net[k].reshape(-1) for k in ("w_ih", "w_hh", "b_ih", "b_hh")]
    parts += [a.reshape(-1) for w, b in zip(net["w"], net["b"]) for a in (w, b)]
    if actor:
        parts.append(net["log_std"].reshape(-1))
    return np.concatenate(parts).astype(np.float32)


def unflat(vec, like, actor):
    """The inverse of ``flat``: a network of ``like``'s shapes from a flat row."""
    vec = np.asarray(vec, np.float32)
    H = L.hidden_of(like)
    shapes = [(4 * H, IN), (4 * H, H), (4 * H,), (4 * H,)]
    for w in like["w"]:
        shapes += [tuple(w.shape), (w.shape[0],)]
    out, at = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(vec[at:at + n].reshape(s).copy()); at += n
    log_std = vec[at:at + OUT].copy() if actor else None
    assert at + (OUT if actor else 0) == vec.size, (at, vec.size)
    return L.make_net(out[0], out[1], out[2], out[3], out[4::2], out[5::2], like["act"], log_std)


def grad_floats(net, actor):
    return flat(net, actor).size


# ------------------------------------------------------------------------------------------------------------ the packer, restated
def _split16(x, s):
    """x 2^s = hi + lo as two float16 (round to nearest even, subnormals kept), as uint16 bit patterns"""
    ws = np.ldexp(np.asarray(x, np.float32), s).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = ws.astype(np.float16)
        lo = (ws - hi.astype(np.float32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def _fragments(w, MT, KS, natural, shifts):
    """[2, MT, KS, 64, 8] uint16: the fragments [term][mt][ks] of the matrix w (zero-padded to 32 MT rows and 16 KS columns); ``shifts``:
    one shift, or one per k-step"""
    wp = np.zeros((32 * MT, 16 * KS), np.float32)
    wp[:w.shape[0], :w.shape[1]] = w
    lane, j, ks = np.arange(64), np.arange(8), np.arange(KS)
    r, h = lane & 31, lane >> 5
    if natural:
        k = 16 * ks[:, None, None] + 8 * h[None, :, None] + j[None, None, :]
    else:
        k = (32 * (ks >> 1) + 16 * (ks & 1))[:, None, None] + 8 * (j >> 2)[None, None, :] + 4 * h[None, :, None] + (j & 3)[None, None, :]
    rows = 32 * np.arange(MT)[:, None, None, None] + r[None, None, :, None]
    vals = wp[rows, k[None]]                                       # [MT, KS, 64, 8]
    shifts = np.broadcast_to(np.asarray(shifts, np.int32), (KS,))
    out = np.zeros((2, MT, KS, 64, 8), np.uint16)
    for q in range(KS):
        out[0, :, q], out[1, :, q] = _split16(vals[:, q], int(shifts[q]))
    return out


def _biases(b, MT, s):
    """[MT, 2, 16] float32: the biases in accumulator order times 2^(10 + s); padded rows zero"""
    bp = np.zeros(32 * MT, np.float32)
    bp[:b.size] = b
    e, h = np.arange(16), np.arange(2)
    rows = 32 * np.arange(MT)[:, None, None] + ((e & 3) + 8 * (e >> 2))[None, None, :] + 4 * h[None, :, None]
    return (bp[rows] * f32(2.0 ** (X_SHIFT + s))).astype(np.float32)


def cell_shifts(net):
    return R.documented_shift(net["w_ih"]), R.documented_shift(net["w_hh"])


def pack_block(net, actor, separate_shifts=False):
    """The block [trunk block | cell block] of a recurrent handle, float32 [block_floats], as pack_lstm_weights builds it — but for the six
    exp(log_std) floats, which are float32(exp(float64(log_std))) here (the device repack's expression).  ``separate_shifts``: the WRONG
    restatement that scales W_ih and W_hh by their own shifts (the cell's inverse scale then follows W_hh's)."""
    H = L.hidden_of(net)
    ws, bs = net["w"], net["b"]
    n_layers = len(ws)
    mt = [2 if w.shape[0] == 64 and l < n_layers - 1 else 1 for l, w in enumerate(ws)]
    ks = [w.shape[1] // 16 for w in ws]
    frag0 = np.concatenate([[0], np.cumsum([2 * m * k for m, k in zip(mt, ks)])]).astype(int)
    tile0 = np.concatenate([[0], np.cumsum(mt)]).astype(int)
    bias0 = MLP_HDR + int(frag0[-1]) * FRAG_FLOATS
    trunk_total = bias0 + int(tile0[-1]) * 32
    tiles, KS = 4 * (H // 32), 2 + H // 16
    cell_floats = CELL_HDR + 2 * tiles * KS * FRAG_FLOATS + 2 * tiles * 32
    block = np.zeros(trunk_total + cell_floats, np.float32)
    words = block.view(np.int32)
    words[0:6] = [n_layers - 1, ACT_CODES[net["act"]], ws[-1].shape[0], trunk_total, H, trunk_total]
    halves = block.view(np.uint16)
    for l, (w, b) in enumerate(zip(ws, bs)):
        s = R.documented_shift(w)
        fr = _fragments(w, mt[l], ks[l], l == 0, s)
        at = 2 * (MLP_HDR + int(frag0[l]) * FRAG_FLOATS)
        halves[at:at + fr.size] = fr.reshape(-1)
        bias_at = bias0 + int(tile0[l]) * 32
        block[bias_at:bias_at + mt[l] * 32] = _biases(b, mt[l], s).reshape(-1)
        rec = MLP_REC + MLP_REC_STRIDE * l
        words[rec:rec + 4] = [int(frag0[l]), bias_at, mt[l], ks[l]]
        block[rec + 4] = f32(2.0 ** -(X_SHIFT + s))
    if actor:
        block[MLP_STD:MLP_STD + OUT] = np.exp(net["log_std"].astype(np.float64)).astype(np.float32)
        block[MLP_STD + 8:MLP_STD + 8 + OUT] = net["log_std"]
    # the cell: [W_ih | W_hh] as ONE matrix of 4 H rows over 32 (17 used) + H columns in natural k order; tile t holds rows 32 t .. 32 t + 31
    s_ih, s_hh = cell_shifts(net)
    s = min(s_ih, s_hh)
    both = np.zeros((4 * H, 32 + H), np.float32)
    both[:, :IN], both[:, 32:] = net["w_ih"], net["w_hh"]
    shifts = [s_ih, s_ih] + [s_hh] * (H // 16) if separate_shifts else s
    if separate_shifts:
        s = s_hh
    cell = block[trunk_total:]
    cell[0] = f32(2.0 ** -(X_SHIFT + s))
    cell.view(np.int32)[1] = H
    fr = _fragments(both, tiles, KS, True, shifts)
    cell.view(np.uint16)[2 * CELL_HDR:2 * CELL_HDR + fr.size] = fr.reshape(-1)
    cb = CELL_HDR + 2 * tiles * KS * FRAG_FLOATS
    cell[cb:cb + tiles * 32] = _biases(net["b_ih"], tiles, s).reshape(-1)
    cell[cb + tiles * 32:cb + 2 * tiles * 32] = _biases(net["b_hh"], tiles, s).reshape(-1)
    return block


def cell_of(block):
    """The cell block of a packed block (header word 5: its float offset)"""
    return block[int(block.view(np.int32)[5]):]


def unpack_cell(block, H):
    """(W_ih [4H,17], W_hh [4H,H]) in float64 as the matrix cores see them: (hi + lo) times the block's own inverse weight scale"""
    cell = cell_of(block)
    tiles, KS = 4 * (H // 32), 2 + H // 16
    s = -int(np.round(np.log2(float(cell[0])))) - X_SHIFT
    fr = cell.view(np.uint16)[2 * CELL_HDR:2 * CELL_HDR + 2 * tiles * KS * 512].reshape(2, tiles, KS, 64, 8).view(np.float16).astype(np.float64)
    q = fr[0] + fr[1]                                              # [tiles, KS, 64, 8]
    both = np.zeros((4 * H, 32 + H))
    lane, j = np.arange(64), np.arange(8)
    r, h = lane & 31, lane >> 5
    for t in range(tiles):
        for k in range(KS):
            both[(32 * t + r)[:, None], (16 * k + 8 * h)[:, None] + j[None, :]] = q[t, k]
    both = np.ldexp(both, -s)
    return both[:, :IN], both[:, 32:], s


# ------------------------------------------------------------------------------------------------------------ corners of the ONE shift
def corner_net(which, H=32, arch=(16,), act="tanh", seed=7):
    """An actor whose cell reaches a corner of min(s_ih, s_hh):
      "hh_dominates"    max |W_hh| = 40 (shift 9), W_ih below 1 (shift 10): the shift is W_hh's;
      "ih_dominates"    max |W_ih| = 300 (shift 6), W_hh below 1: the shift is W_ih's;
      "negative_shift"  max |W_hh| = 2^16 (shift -2): a shift below zero;
      "zero_lstm"       W_ih = W_hh = 0 with a non-zero trunk: shift 10, zero fragments."""
    net = L.hot(H, arch, act, seed=seed)
    w_ih, w_hh = net["w_ih"].copy(), net["w_hh"].copy()
    w_ih *= f32(0.9) / np.abs(w_ih).max()
    w_hh *= f32(0.9) / np.abs(w_hh).max()
    if which == "hh_dominates":
        w_hh[5, 3] = f32(-40.0)
    elif which == "ih_dominates":
        w_ih[4 * H - 1, 16] = f32(300.0)
    elif which == "negative_shift":
        w_hh[H + 1, H - 1] = f32(2.0 ** 16)
    elif which == "zero_lstm":
        w_ih, w_hh = np.zeros_like(w_ih), np.zeros_like(w_hh)
    else:
        raise KeyError(which)
    return L.make_net(w_ih, w_hh, net["b_ih"], net["b_hh"], net["w"], net["b"], act, np.linspace(-1.0, 0.5, OUT))


CORNER_SHIFTS = {"hh_dominates": (10, 9), "ih_dominates": (6, 10), "negative_shift": (10, -2), "zero_lstm": (10, 10)}


# ------------------------------------------------------------------------------------------------------------ comparing blocks
def blocks_equal(got, want, actor):
    """A block the device repacked against the host packer's (float32 arrays): byte for byte outside the six exp(log_std) floats of an
    actor block; those within 1 ulp of float32(exp(float64(log_std))) and within 2 ulp of the host block's.  A message, or None."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    a, b = got.view(np.uint32), want.view(np.uint32)
    if a.shape != b.shape:
        return f"{a.shape} against {b.shape} floats"
    same = a == b
    if actor:
        same[MLP_STD:MLP_STD + OUT] = True
    if not same.all():
        at = np.flatnonzero(~same)
        return f"{at.size} words differ, first at float {int(at[0])}: {a[at[0]]:#010x} != {b[at[0]]:#010x}"
    if actor:
        std, log_std = got[MLP_STD:MLP_STD + OUT].astype(np.float64), got[MLP_STD + 8:MLP_STD + 8 + OUT]
        exact = np.exp(log_std.astype(np.float64)).astype(np.float32)
        if not (np.abs(std - exact.astype(np.float64)) <= A.ulp(exact)).all():
            return f"exp(log_std) {std} is not within 1 ulp of {exact}"
        host = want[MLP_STD:MLP_STD + OUT]
        if not (np.abs(std - host.astype(np.float64)) <= 2.0 * A.ulp(host)).all():
            return f"exp(log_std) {std} is not within 2 ulp of the host block's {host}"
    return None
