"""What the two tables of the convolution family (tests/test_gpu_conv_fp32.py, tests/test_gpu_conv_bf16.py) share: the
row of a table and its geometry, the drawing of the operands with their references from tests/conv_ref.py, torch's CPU
fp32 result of the same launch, weight packing, guarded destinations and the launches through the C ABI (mseg_igemm,
mseg_wgrad and their _query twins).  A plain helper module: no tests, no fixtures.

A row's `opt` may say how the launch is typed: prec ("f32" | "bf16": MsegIgemm.precision / MsegWgrad.precision), sdt / ddt
("f32" | "bf16": storage of the sources / of the destinations), stats (None | "none" | "relu": MsegIgemm.stats is set and
stats_act is that activation).  With prec == "bf16" the operands of the reference are rounded the way the kernels round
them (conv_ref.operand_bf16; weights directly) and the data carries the widening `wid` of every output element."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as CR
import pointwise_ref as R

U = 2.0 ** -24
TINY = 2.0 ** -100
GUARD = 256
SENT = np.array([0xFFC12345], dtype=np.uint32).view(np.int32)[0]      # a NaN no kernel produces
NANBITS = np.array([0x7FC00000], dtype=np.uint32).view(np.int32)[0]
SENT16 = np.array([0xFFA5], dtype=np.uint16).view(np.int16)[0]        # 16-bit storage: a NaN pattern no conversion gives
NANBITS16 = np.array([0x7FC0], dtype=np.uint16).view(np.int16)[0]
EINVAL = -1
GENERIC = ("leakyrelu", "elu", "mish")


def _b(v):
    return "true" if v else "false"


Row = collections.namedtuple("Row", "id op N cs Co H W stride acts tabs dest kernel xkernel opt")


def row(id, op, N, cs, Co, H, W, kernel, xkernel=None, stride=1, acts=None, tabs=None, dest="plain", **opt):
    """op: conv (3x3 forward), dgrad (its data gradient, TCONV), convT (ConvTranspose 2x2, scatter), convT_dgrad, wgrad3
    (3x3 weight gradient), wgrad2 (ConvTranspose weight gradient).  cs: channels of the GEMM's sources (for the weight
    gradients: of Q); Co: output channels (convT: Cq; weight gradients: channels of P).  H, W: size of the sources (weight
    gradients: of P).  acts / tabs: per source the activation and the table kind (None, "c" per channel, "s" per sample).
    dest: plain | ld (padded leading dimension, opt ldpad) | acc | split (opt split: first part accumulates, second does not).
    opt: pact / ptab (transform of P), out_hw / q_hw (size of the output / of Q where it is not the default), parity, splits,
    nch_store, bias, ws_off (bytes the weight-gradient workspace is moved off its 16-byte alignment); prec, sdt, ddt, stats
    (module docstring)."""
    acts = list(acts) if acts else ["none"] * len(cs)
    tabs = list(tabs) if tabs else [None] * len(cs)
    assert len(acts) == len(cs) == len(tabs)
    return Row(id, op, N, list(cs), Co, H, W, stride, acts, tabs, dest, kernel, xkernel or kernel, opt)


# =================================================================================================================================
# geometry of a row
# =================================================================================================================================
def is_wgrad(r):
    return r.op.startswith("wgrad")


def is_bf16(r):
    return r.opt.get("prec", "f32") == "bf16"


def geom(r):
    g = {}
    if r.op == "conv":
        g.update(Hi=r.H, Wi=r.W, Ho=CR.out_size(r.H, r.stride), Wo=CR.out_size(r.W, r.stride), K=3, stride=r.stride, pad=1,
                 mode=0, Ngemm=r.Co, epi=0, Cq=0, T=9)
    elif r.op == "dgrad":
        Ho, Wo = r.opt.get("out_hw", (r.H, r.W) if r.stride == 1 else (2 * r.H, 2 * r.W))
        g.update(Hi=r.H, Wi=r.W, Ho=Ho, Wo=Wo, K=3, stride=r.stride, pad=1, mode=1, Ngemm=r.Co, epi=0, Cq=0, T=9)
    elif r.op == "convT":
        g.update(Hi=r.H, Wi=r.W, Ho=r.H, Wo=r.W, K=1, stride=1, pad=0, mode=0, Ngemm=4 * r.Co, epi=1, Cq=r.Co, T=1)
    elif r.op == "convT_dgrad":
        g.update(Hi=r.H, Wi=r.W, Ho=r.H // 2, Wo=r.W // 2, K=2, stride=2, pad=0, mode=0, Ngemm=r.Co, epi=0, Cq=0, T=4)
    elif r.op == "wgrad3":
        Hq, Wq = r.opt.get("q_hw", (r.H, r.W) if r.stride == 1 else (2 * r.H, 2 * r.W))
        g.update(Hp=r.H, Wp=r.W, Hq=Hq, Wq=Wq, K=3, stride=r.stride, pad=1)
    elif r.op == "wgrad2":
        g.update(Hp=r.H, Wp=r.W, Hq=2 * r.H, Wq=2 * r.W, K=2, stride=2, pad=0)
    else:
        raise ValueError(r.op)
    if not is_wgrad(r):
        g["morder"] = 1 if (r.op == "dgrad" and r.opt.get("parity", r.stride == 2)) else 0
        g["Cin"] = sum(r.cs)
        g["Kpad"], g["Npad"] = -(-g["Cin"] // 32) * 32, -(-g["Ngemm"] // 128) * 128
        g["out_rows"] = r.N * g["Ho"] * g["Wo"] * (4 if r.op == "convT" else 1)
        g["out_cols"] = r.Co
        g["bias"] = r.opt.get("bias", r.op in ("conv", "convT"))
        n = g["Ngemm"]
        if r.dest == "split":
            c0 = r.opt["split"]
            g["dsts"] = [(c0, c0, 1), (n - c0, n - c0, 0)]           # (columns, leading dimension, accumulate)
        elif r.dest == "ld":
            g["dsts"] = [(r.Co, r.Co + r.opt["ldpad"], 0)]
        else:
            g["dsts"] = [(r.Co, r.Co, 1 if r.dest == "acc" else 0)]
        g["dot"] = g["T"] * g["Cin"]
    else:
        g["Nch"] = sum(r.cs)
        g["Nst"] = r.opt.get("nch_store", g["Nch"])
        g["dot"] = r.N * g["Hp"] * g["Wp"]
    return g


def epilogue_row_mode(r):
    """which addressing mode of igemm_epilogue a row's launch uses: 0 affine, 1 halo tiles narrower than 32, 2 scatter over
    rows that are no multiple of 32, 3 parity order inside a class, 4 a 32-row tile straddling two parity classes.
    The library does not report the mode: this RESTATES the selection in microbeseg_amd/csrc/igemm_common.h, igemm_epilogue,
    the block `if (tw_log2 >= 0) ... else if (e_epi == MSEG_EPI_SCATTER2X2) ... else if (e_morder == MSEG_MORDER_PARITY)`
    that sets `mode` (lines 136-167 when this was written), and the tile width of halo_geometry() in igemm.hip (largest
    power of two <= 64 dividing W).  It will not notice a change there: keep the two in step."""
    g = geom(r)
    if r.kernel.startswith("igemm_halo_kernel"):
        tw = 64
        while r.W % tw:
            tw //= 2
        return 0 if tw >= 32 else 1
    if g["epi"] == 1:
        return 0 if g["Wo"] % 32 == 0 else 2
    if g["morder"] == 1:
        if (g["Wo"] // 2) % 32 == 0:
            return 0
        per = r.N * g["Ho"] * g["Wo"] // 4
        return 3 if per % 32 == 0 else 4
    return 0


def float_variants(r):
    """(acts, pact) combinations of the float mode: every activation the row's kernel takes"""
    pact, ptab = r.opt.get("pact", "none"), r.opt.get("ptab")
    allacts = r.acts + [pact]
    if any(a in GENERIC for a in allacts):
        out = []
        for gact in GENERIC:
            v = [gact if a in GENERIC else a for a in allacts]
            out.append((v[:-1], v[-1]))
        return out
    swap = {"none": "relu", "relu": "none"}
    v = [swap[a] if t else a for a, t in zip(allacts, r.tabs + [ptab])]     # a table keeps the transform alive
    out = [(r.acts, pact)]
    if v != allacts:
        out.append((v[:-1], v[-1]))
    return out


def exact_acts(r):
    fix = lambda a: "relu" if a in GENERIC else a
    return [fix(a) for a in r.acts], fix(r.opt.get("pact", "none"))


# =================================================================================================================================
# descriptors
# =================================================================================================================================
def _eng():
    from microbeseg_amd import engine, _lib
    return engine, _lib, _lib.load()


def _src(ptr, Cc, act, tab, scale_ptr=256, shift_ptr=256, dtype=0):
    from microbeseg_amd._lib import MsegSrc, ACT
    s = MsegSrc()
    s.ptr, s.C, s.act, s.dtype = ptr, Cc, ACT[act], dtype
    if tab:
        s.scale, s.shift, s.ss = scale_ptr, shift_ptr, (Cc if tab == "s" else 0)
    return s


def _st(r, key):
    return 1 if r.opt.get(key, "f32") == "bf16" else 0


def engine_query(r, acts, pact):
    """engine.igemm_query / engine.wgrad_query for the row (placeholder pointers: needs the library, no device)"""
    engine, _, _ = _eng()
    g = geom(r)
    sdt, prec = _st(r, "sdt"), r.opt.get("prec", "f32")
    srcs = [_src(256, c, a, t, dtype=sdt) for c, a, t in zip(r.cs, acts, r.tabs)]
    if is_wgrad(r):
        P = _src(256, r.Co, pact, r.opt.get("ptab"), dtype=sdt)
        return engine.wgrad_query(P, srcs, r.N, g["Hp"], g["Wp"], g["Hq"], g["Wq"], g["K"], g["K"], g["stride"], g["pad"],
                                  nch_store=g["Nst"], precision=prec)
    d = g["dsts"]
    return engine.igemm_query(srcs, g["Kpad"], g["Npad"], r.N, g["Hi"], g["Wi"], g["Ho"], g["Wo"], g["K"], g["K"], g["stride"],
                              g["pad"], g["mode"], g["Ngemm"], d[0][1], acc0=d[0][2], ld1=d[1][1] if len(d) > 1 else 0,
                              acc1=0, split=d[0][0] if len(d) > 1 else None, epi=g["epi"], Cq=g["Cq"], morder=g["morder"],
                              precision=prec, dst_dtype=_st(r, "ddt"), bias=g["bias"])


# =================================================================================================================================
# data and references
# =================================================================================================================================
def _tables(rng, mode, tab, N, Cc):
    if not tab:
        return None, None
    shape = (N, Cc) if tab == "s" else (Cc,)
    if mode == "exact":
        sc = rng.choice([-2, -1, 1, 2, 3], size=shape)
        sh = rng.choice([-2, -1, 1, 2], size=shape)             # never 0: a transformed padding pixel is not 0
    else:
        sc, sh = 1.0 + 0.3 * rng.normal(size=shape), 0.5 * rng.normal(size=shape)
    return sc.astype(np.float32), sh.astype(np.float32)


def _draw(rng, mode, shape, sigma=1.0, quick=False):
    """quick (the bf16 table, whose gate-sized rows hold 3e7 elements): the same distributions drawn in 8 / 32 bits"""
    if mode == "exact":
        if quick:
            return rng.integers(-3, 4, size=shape, dtype=np.int8).astype(np.float32)
        return rng.integers(-3, 4, size=shape).astype(np.float32)
    if quick:
        return np.float32(sigma) * rng.standard_normal(size=shape, dtype=np.float32)
    return (sigma * rng.normal(size=shape)).astype(np.float32)


def _stored(v, bf16):
    """the values a tensor of that storage holds: fp32 as drawn, or their bf16 rounding (still a float32 array)"""
    return CR.round_bf16(v).astype(np.float32) if bf16 else v


def _minus_zeros(rng, z):
    """exact mode of the bf16 table: every third zero becomes -0.0 (ReLU on the bf16 bit pattern must still give 0)"""
    hit = (z == 0) & (rng.integers(0, 3, size=z.shape, dtype=np.int8) == 0)
    z[hit] = np.float32(-0.0)
    return z


def make_data(r, mode, acts, pact, seed, want_ref=True):
    """host arrays of one launch (fp32 values; what a bf16 tensor holds is exactly representable) and the reference of
    conv_ref: fp64, or int64 in the exact mode -> dict.  bf16 rows: the operands are the kernels' bf16 operands and d['wid']
    is the widening of every output element (module docstring).  want_ref = False: only S and wid (the host test)."""
    if not want_ref:
        CR.MAGNITUDES_ONLY = True
        try:
            d = make_data(r, mode, acts, pact, seed)
        finally:
            CR.MAGNITUDES_ONLY = False
        d.pop("ref")
        return d
    rng = np.random.Generator(np.random.PCG64(seed))
    g = geom(r)
    b16, s16, d16 = is_bf16(r), _st(r, "sdt") == 1, _st(r, "ddt") == 1
    d = {"acts": acts, "pact": pact, "mode": mode}
    sizes = [(g["Hq"], g["Wq"])] * len(r.cs) if is_wgrad(r) else [(g["Hi"], g["Wi"])] * len(r.cs)
    d["z"], d["sc"], d["sh"] = [], [], []
    for i, (c, t, hw) in enumerate(zip(r.cs, r.tabs, sizes)):
        z = _draw(rng, mode, (r.N, hw[0], hw[1], c), quick=b16)
        if mode == "float" and i == 0:
            z[..., 0] += np.float32(1.5)
        if b16 and mode == "exact":
            z = _minus_zeros(rng, z)
        sc, sh = _tables(rng, mode, t, r.N, c)
        d["z"].append(_stored(z, s16)), d["sc"].append(sc), d["sh"].append(sh)
    # exact mode: the operands are checked to be integers (as_exact) and the sums are formed in fp64, which is exact for
    # integers below 2^53 and runs through BLAS (numpy's int64 matmul does not); the results go back to int64 below
    cast = (lambda v: CR.as_exact(v).astype(np.float64)) if mode == "exact" else (lambda v: v)
    if b16:
        pairs = [CR.operand_bf16(z, a, sc, sh) for z, a, sc, sh in zip(d["z"], acts, d["sc"], d["sh"])]
        ops, amb = [cast(p[0]) for p in pairs], [p[1] for p in pairs]
    else:
        ops = [cast(CR.operand(z, a, sc, sh)) for z, a, sc, sh in zip(d["z"], acts, d["sc"], d["sh"])]
        amb = None
    d["ops"] = ops
    wid = None
    if is_wgrad(r):
        pz = _draw(rng, mode, (r.N, g["Hp"], g["Wp"], r.Co), quick=b16)
        if b16 and mode == "exact":
            pz = _minus_zeros(rng, pz)
        d["pz"] = _stored(pz, s16)
        d["psc"], d["psh"] = _tables(rng, mode, r.opt.get("ptab"), r.N, r.Co)
        if b16:
            P, PA = CR.operand_bf16(d["pz"], pact, d["psc"], d["psh"])
            P = cast(P)
        else:
            P, PA = cast(CR.operand(d["pz"], pact, d["psc"], d["psh"])), None
        d["P"] = P
        d["ref"], d["S"] = CR.wgrad(P, ops, g["K"], g["stride"], g["Nst"])
        if b16:
            wid = np.zeros(d["S"].shape)
            absf = lambda v: np.abs(np.asarray(v, dtype=np.float64))
            if any(a.any() for a in amb):
                wid += CR.wgrad(absf(P), amb, g["K"], g["stride"], g["Nst"])[0]
            if PA.any():
                wid += CR.wgrad(PA, [absf(o) for o in ops], g["K"], g["stride"], g["Nst"])[0]
    else:
        Cin, n = g["Cin"], g["Ngemm"]
        sig = 1.0 if mode == "exact" else 1.0 / np.sqrt(g["T"] * Cin)
        wshape = {"conv": (r.Co, Cin, 3, 3), "dgrad": (Cin, r.Co, 3, 3), "convT": (Cin, r.Co, 2, 2),
                  "convT_dgrad": (r.Co, Cin, 2, 2)}[r.op]
        d["w"] = w = _stored(_draw(rng, mode, wshape, sig), b16)       # bf16 launches take the bf16 copy of the weights
        d["bias"] = bias = _draw(rng, mode, (r.Co,)) if g["bias"] else None
        # exact mode with a bf16 destination: the bias and the old content of an accumulating destination lift the sums
        # beyond 256, where only every second integer is a bf16 value: odd sums are rounding ties, so a store that
        # truncates or rounds half up gives other bits than round-to-nearest-even
        lift = mode == "exact" and d16
        if lift and bias is not None:
            d["bias"] = bias = (rng.integers(257, 320, size=(r.Co,)) * rng.choice([-1, 1], size=(r.Co,))).astype(np.float32)
        rows, cols = g["out_rows"], g["out_cols"]
        base = np.zeros((rows, cols), dtype=np.float32)
        c = 0
        for (k, _, acc) in g["dsts"]:
            if acc:
                base[:, c:c + k] = _stored(_draw(rng, mode, (rows, k), quick=b16), d16)
                if lift:                                                # even, 258 .. 318: bf16 values
                    base[:, c:c + k] = 2 * rng.integers(129, 160, size=(rows, k), dtype=np.int16) * np.sign(base[:, c:c + k] + 0.5)
            c += k
        d["base"] = base
        oshape = (r.N, g["Ho"] * (2 if r.op == "convT" else 1), g["Wo"] * (2 if r.op == "convT" else 1), r.Co)
        wc, bc, basec = cast(w), (None if bias is None else cast(bias)), cast(base).reshape(oshape)

        def apply(xs, wv, bv, bs):
            if r.op == "conv":
                return CR.conv_fwd(xs, wv, bv, r.stride, bs)
            if r.op == "convT":
                return CR.convT_fwd(np.concatenate(xs, 3), wv, bv, bs)
            if r.op == "dgrad":
                out, S = CR.conv_dgrad(np.concatenate(xs, 3), wv, r.stride, g["Ho"], g["Wo"], bs)
            else:
                out, S = CR.convT_dgrad(np.concatenate(xs, 3), wv, bs)
            if bv is not None:                                          # a data gradient launched with a bias (opt bias)
                out, S = out + np.asarray(bv).astype(out.dtype), S + np.abs(np.asarray(bv)).astype(S.dtype)
            return out, S

        ref = apply(ops, wc, bc, basec)
        d["ref"], d["S"] = ref[0].reshape(rows, cols), ref[1].reshape(rows, cols)
        if b16:
            if any(a.any() for a in amb):
                wid = apply(amb, np.abs(w).astype(np.float64), None, None)[0].reshape(rows, cols)
            else:
                wid = np.zeros(d["S"].shape)
    if b16:
        d["wid"] = wid
    if mode == "exact":
        d["ref"], d["S"] = CR.as_exact(d["ref"]), CR.as_exact(d["S"])
        CR.assert_exact(d["S"])
        assert wid is None or not wid.any()
    return d


def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _op32(z, act, sc, sh):
    """the operand as fp32 arithmetic computes it, NCHW"""
    a = R.activation(_t32(z), act, dtype=torch.float32)
    if sc is not None:
        s, h = _t32(sc), _t32(sh)
        if s.dim() == 1:
            s, h = s[None], h[None]
        a = a * s[:, None, None, :] + h[:, None, None, :]
    return a.permute(0, 3, 1, 2).contiguous()


def _nchw32(a):
    return _t32(np.asarray(a, dtype=np.float32)).permute(0, 3, 1, 2).contiguous()


def torch_fp32(r, d):
    """torch's CPU fp32 result of the same operation on the same inputs (bf16 rows: on the same bf16-rounded operands, which
    fp32 holds exactly), shaped like d['ref']"""
    g = geom(r)
    if is_bf16(r):
        x = torch.cat([_nchw32(o) for o in d["ops"]], 1)
    else:
        x = torch.cat([_op32(z, a, sc, sh) for z, a, sc, sh in zip(d["z"], d["acts"], d["sc"], d["sh"])], 1)
    if is_wgrad(r):
        P = _nchw32(d["P"]) if is_bf16(r) else _op32(d["pz"], d["pact"], d["psc"], d["psh"])
        if r.op == "wgrad3":
            w = torch.zeros(r.Co, g["Nch"], 3, 3, requires_grad=True)
            F.conv2d(x, w, None, stride=r.stride, padding=1).backward(P)
        else:
            w = torch.zeros(r.Co, g["Nch"], 2, 2, requires_grad=True)
            F.conv_transpose2d(P, w, None, stride=2).backward(x)
        return w.grad[:, :g["Nst"]].numpy()
    w = _t32(d["w"])
    b = None if d["bias"] is None else _t32(d["bias"])
    if r.op == "conv":
        y = F.conv2d(x, w, b, stride=r.stride, padding=1)
    elif r.op == "dgrad":
        xin = torch.zeros(r.N, r.Co, g["Ho"], g["Wo"], requires_grad=True)
        F.conv2d(xin, w, None, stride=r.stride, padding=1).backward(x)
        y = xin.grad if b is None else xin.grad + b[None, :, None, None]
    elif r.op == "convT":
        y = F.conv_transpose2d(x, w, b, stride=2)
    else:
        xin = torch.zeros(r.N, r.Co, g["Ho"], g["Wo"], requires_grad=True)
        F.conv_transpose2d(xin, w, None, stride=2).backward(x)
        y = xin.grad if b is None else xin.grad + b[None, :, None, None]
    y = y.detach().permute(0, 2, 3, 1).reshape(g["out_rows"], g["out_cols"])
    return (y + _t32(d["base"])).numpy()


def pack_weight(r, w):
    """[T][Npad][Kpad] GEMM operand of include/mseg_hip.h, zero filled, from the torch-layout weight"""
    g = geom(r)
    perm = {"conv": (2, 3, 0, 1), "dgrad": (2, 3, 1, 0), "convT": (2, 3, 1, 0), "convT_dgrad": (2, 3, 0, 1)}[r.op]
    T = 1 if r.op == "convT" else g["K"] * g["K"]
    core = np.transpose(w, perm).reshape(T, g["Ngemm"], g["Cin"])
    wp = np.zeros((T, g["Npad"], g["Kpad"]), dtype=np.float32)
    wp[:, :g["Ngemm"], :g["Cin"]] = core
    return wp


# =================================================================================================================================
# guarded buffers and launches
# =================================================================================================================================
def _sync():
    """wait for the device; a HIP error here (a faulted kernel) ends the whole session: nothing more is started on that device"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"HIP error after a launch, stopping: {e}", returncode=3)


def _dev(a, bf16=False):
    """host fp32 array -> device tensor of that storage (the values of a bf16 tensor are representable: no rounding here)"""
    t = _t32(a).cuda()
    return t.to(torch.bfloat16) if bf16 else t


class Guarded:
    """rows x cols values at leading dimension ld inside sentinels: GUARD words before and after, and the columns cols .. ld.
    bf16 = True: 16-bit words (every check below is then made per 2-byte word)."""

    def __init__(self, rows, cols, ld, init=None, bf16=False):
        self.rows, self.cols, self.ld, self.bf16 = rows, cols, ld, bf16
        word, sent, nan = (np.int16, SENT16, NANBITS16) if bf16 else (np.int32, SENT, NANBITS)
        host = np.full(GUARD + rows * ld + GUARD, sent, dtype=word)
        body = host[GUARD:GUARD + rows * ld].reshape(rows, ld)
        if init is None:
            body[:, :cols] = nan
        elif bf16:
            bits = np.ascontiguousarray(init, dtype=np.float32).view(np.uint32)
            assert not (bits & 0xFFFF).any(), "the initial content of a bf16 destination must be bf16 values"
            body[:, :cols] = (bits >> 16).astype(np.uint16).view(np.int16)
        else:
            body[:, :cols] = np.ascontiguousarray(init, dtype=np.float32).view(np.int32)
        self.before = host.copy()
        self.dev = torch.from_numpy(host).cuda()
        self.ptr = self.dev.data_ptr() + host.itemsize * GUARD

    def take(self):
        """-> the values (fp32, host) after checking every sentinel bit for bit"""
        _sync()
        after = self.dev.cpu().numpy()
        mask = np.ones(after.shape, dtype=bool)
        mask[GUARD:GUARD + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols] = False
        bad = np.nonzero(mask & (after != self.before))[0]
        assert bad.size == 0, f"{bad.size} sentinel words overwritten, first at word {int(bad[0]) - GUARD} of the destination"
        body = after[GUARD:GUARD + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols].copy()
        if self.bf16:
            return (body.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
        return body.view(np.float32)

    def untouched(self):
        _sync()
        return np.array_equal(self.dev.cpu().numpy(), self.before)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _name(lib, fn, p):
    from microbeseg_amd._lib import MsegKernelInfo
    info = MsegKernelInfo()
    rc = fn(C.byref(p), C.byref(info))
    return rc, info


def _dev_srcs(r, d, keep):
    out = []
    s16 = _st(r, "sdt")
    for c, z, a, t, sc, sh in zip(r.cs, d["z"], d["acts"], r.tabs, d["sc"], d["sh"]):
        zt = _dev(z, s16)
        keep.append(zt)
        if t:
            st, ht = _t32(sc).cuda(), _t32(sh).cuda()
            keep += [st, ht]
            out.append(_src(zt.data_ptr(), c, a, t, st.data_ptr(), ht.data_ptr(), dtype=s16))
        else:
            out.append(_src(zt.data_ptr(), c, a, None, dtype=s16))
    return out


def build_igemm(r, d, keep):
    """the descriptor the way engine.igemm builds it (split-K scratch from mseg_igemm_workspace_bytes included) -> (p, dsts)"""
    _, L, lib = _eng()
    g = geom(r)
    p = L.MsegIgemm()
    for i, s in enumerate(_dev_srcs(r, d, keep)):
        p.src[i] = s
    p.nsrc, p.Cin, p.Kpad, p.Npad = len(r.cs), g["Cin"], g["Kpad"], g["Npad"]
    p.NB, p.Hi, p.Wi, p.Ho, p.Wo = r.N, g["Hi"], g["Wi"], g["Ho"], g["Wo"]
    p.KH = p.KW = g["K"]
    p.stride, p.pad, p.mode, p.morder = g["stride"], g["pad"], g["mode"], g["morder"]
    p.Ngemm, p.epi, p.Cq = g["Ngemm"], g["epi"], g["Cq"]
    p.precision, p.dst_dtype = (1 if is_bf16(r) else 0), _st(r, "ddt")
    wt = _dev(pack_weight(r, d["w"]), is_bf16(r))
    keep.append(wt)
    p.w = wt.data_ptr()
    if d["bias"] is not None:
        bt = _t32(d["bias"]).cuda()
        keep.append(bt)
        p.bias = bt.data_ptr()
    dsts, c = [], 0
    for (k, ld, acc) in g["dsts"]:
        dsts.append(Guarded(g["out_rows"], k, ld, d["base"][:, c:c + k] if acc else None, bf16=_st(r, "ddt") == 1))
        c += k
    p.dst0, p.ld0, p.acc0 = dsts[0].ptr, g["dsts"][0][1], g["dsts"][0][2]
    p.split = g["Ngemm"]
    if len(dsts) > 1:
        p.dst1, p.ld1, p.acc1, p.split = dsts[1].ptr, g["dsts"][1][1], g["dsts"][1][2], g["dsts"][0][0]
    need = lib.mseg_igemm_workspace_bytes(C.byref(p))
    assert (need > 0) == ("splitk" in r.opt), f"split-K scratch {need} bytes"
    if need:
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        keep.append(ws)
        p.ws, p.ws_bytes = ws.data_ptr(), need
    return p, dsts


def run_igemm(r, d, want, stats_out=None):
    """launch the row -> the destinations side by side (fp32 values).  A row with opt `stats` gets a sentinel-filled
    statistics buffer sized by the query's stats_rows (one row where it reports none); stats_out (a dict) receives
    `rows` and `part` ([rows][2][Ngemm], or None when the query reported no rows and the buffer came back untouched)."""
    _, L, lib = _eng()
    keep = []
    p, dsts = build_igemm(r, d, keep)
    sbuf = None
    if r.opt.get("stats"):
        p.stats, p.stats_act = 256, L.ACT[r.opt["stats"]]
    rc, info = _name(lib, lib.mseg_igemm_query, p)
    assert rc == 0 and info.name.decode() == want, (rc, info.name)
    if r.opt.get("stats"):
        n = geom(r)["Ngemm"]
        rows2 = max(info.stats_rows, 1) * 2                              # the body holds sentinels too: every word written shows
        sbuf = Guarded(rows2, n, n, init=np.full((rows2, n), SENT, dtype=np.int32).view(np.float32))
        p.stats = sbuf.ptr
    if "splitk" in r.opt:
        want_ws = r.opt["splitk"] * geom(r)["out_rows"] * geom(r)["Ngemm"] * 4        # one fp32 partial result per split
        assert info.launches >= 2 and info.workspace == want_ws == p.ws_bytes, (info.launches, info.workspace, p.ws_bytes)
    rc = lib.mseg_igemm(C.byref(p), _stream())
    assert rc == 0, f"mseg_igemm returned {rc} (hipError {lib.mseg_last_hip_error()})"
    assert lib.mseg_last_kernel().decode() == want
    out = np.concatenate([b.take() for b in dsts], axis=1)
    if sbuf is not None and stats_out is not None:
        stats_out["rows"] = info.stats_rows
        if info.stats_rows == 0:
            assert sbuf.untouched(), "a launch that reports no statistics rows wrote to the statistics buffer"
            stats_out["part"] = None
        else:
            part = sbuf.take()
            left = int((part.view(np.int32) == SENT).sum())
            assert left == 0, f"{left} words of the {info.stats_rows} statistics rows were not written"
            stats_out["part"] = part.reshape(info.stats_rows, 2, geom(r)["Ngemm"])
    return out


def build_wgrad(r, d, keep):
    _, L, lib = _eng()
    g = geom(r)
    s16 = _st(r, "sdt")
    p = L.MsegWgrad()
    pz = _dev(d["pz"], s16)
    keep.append(pz)
    ptab = r.opt.get("ptab")
    if ptab:
        st, ht = _t32(d["psc"]).cuda(), _t32(d["psh"]).cuda()
        keep += [st, ht]
        p.P = _src(pz.data_ptr(), r.Co, d["pact"], ptab, st.data_ptr(), ht.data_ptr(), dtype=s16)
    else:
        p.P = _src(pz.data_ptr(), r.Co, d["pact"], None, dtype=s16)
    for i, s in enumerate(_dev_srcs(r, d, keep)):
        p.Q[i] = s
    p.nq, p.Nch, p.Nch_store = len(r.cs), g["Nch"], g["Nst"]
    p.NB, p.Hp, p.Wp, p.Hq, p.Wq = r.N, g["Hp"], g["Wp"], g["Hq"], g["Wq"]
    p.KH = p.KW = g["K"]
    p.stride, p.pad = g["stride"], g["pad"]
    p.splits = r.opt.get("splits", 0)
    p.precision = 1 if is_bf16(r) else 0
    need = lib.mseg_wgrad_workspace_bytes(C.byref(p))
    assert need > 0
    off = r.opt.get("ws_off", 0)
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    keep.append(ws)
    assert ws.data_ptr() % 16 == 0 and off % 4 == 0
    p.ws = ws.data_ptr() + off
    dst = Guarded(r.Co, g["Nst"] * g["K"] * g["K"], g["Nst"] * g["K"] * g["K"])
    p.dst = dst.ptr
    if "splits" in r.opt:       # the reduction is chosen by the number of splits the plan ends up with
        per = g["K"] * g["K"] * r.Co * g["Nch"] * 4
        assert need % per == 0 and (need // per >= 32) == (r.opt["splits"] >= 32), need // per
    return p, dst


def run_wgrad(r, d, want):
    _, L, lib = _eng()
    keep = []
    p, dst = build_wgrad(r, d, keep)
    g = geom(r)
    rc, info = _name(lib, lib.mseg_wgrad_query, p)
    assert rc == 0 and info.name.decode() == want, (rc, info.name)
    rc = lib.mseg_wgrad(C.byref(p), _stream())
    assert rc == 0, f"mseg_wgrad returned {rc} (hipError {lib.mseg_last_hip_error()})"
    assert lib.mseg_last_kernel().decode() == want
    return dst.take().reshape(r.Co, g["Nst"], g["K"], g["K"])


def launch(r, d, want, stats_out=None):
    return run_wgrad(r, d, want) if is_wgrad(r) else run_igemm(r, d, want, stats_out)


def family(kernel):
    return kernel.split("<")[0]
