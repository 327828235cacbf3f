"""Every convolution / weight-gradient kernel instance, reached on purpose and checked against a fp64 reference.

lu_conv2d_fwd and lu_conv2d_wgrad choose among ~110 compiled instances by host-side heuristics (patch height, half blocks, narrow
column blocks, halo waste, K-split form, channel tile, pixel stages, LDS-DMA staging, ragged widths, operand element types).  A test
that only picks a shape never learns which instance that shape reached; when a threshold moves, the shape silently drifts to another
instance.  Here each ROW names the instance(s) its descriptor must reach:
  * backend 'emu' (CPU): the host SIMT emulator records every launch (tests/emu/emu_launches.cpp); the record of the row's calls
    must EQUAL the row's expectation, follow-up launches (ksplit_reduce / post_affine / wgrad_reduce) included.  The dispatch is the
    same host code in both builds, so -- with the same pointer alignment, asserted below -- the instance recorded here is the
    instance the MI355X runs for the descriptor;
  * both backends: the result against a fp64 reference of the same operation, at the tolerances of test_kernels.py (fp32: 5e-5 for
    convolutions, 2e-4 for weight gradients; bf16 instances: the fp64 result of the bf16-rounded operands).
Rows sit on edges wherever the instance allows one: frames >= 2, H not a multiple of the patch height, W not a multiple of 32, N
not a multiple of 128 (masked column tiles), C not a multiple of the channel chunk, a bias.  (The bf16 weight-gradient kernels
need W % 32 == 0 and the ConvLSTM epilogue N = 4F with F % 32 == 0: those rows cannot take the W / N edge.)  Flags appear only
where an instance is reachable no other way (or only at shapes far too large for the emulator); the row says why.

test_every_instance_has_a_row / test_instance_list_matches_the_code_object: the committed list tests/golden/dispatch_instances.txt
equals the instances the rows reach and the conv / wgrad / reduce kernel symbols of the built gfx950 code object, so a new
instance without a row fails the suite.
"""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

import kernel_harness as KH
from kernel_harness import bf16_bits, bf16_round, f32
from lu_native import cabi, calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'lstm-unet_amd', 'csrc')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'dispatch_instances.txt')
BACKENDS = ['emu', pytest.param('hip', marks=pytest.mark.gpu)]
CANARY = np.uint32(0x7fa5a5a5)      # a signalling-NaN bit pattern in the padding of strided outputs: must survive bit for bit

# kernel families under the gate: everything lu_conv2d_fwd / lu_conv2d_wgrad (and the stride-2 bf16 entry points) can launch
FAMILY = re.compile(r'^(conv_\w*kernel|wgrad_\w*kernel|ksplit_reduce_kernel|post_affine_kernel)\b')


# ------------------------------------------------------------------------------------------------------------------------
# instance names: the launch sites spell enums and leave default template arguments out; the demangled symbols of the code
# object show numbers and every argument.  Both sides go to the demangled form.
def _template_defaults():
    src = ''.join(open(os.path.join(CSRC, f)).read() for f in ('lu_conv.hip', 'lu_wgrad.hip'))
    consts = {'LU_EPI_BIAS': '0', 'LU_EPI_LSTM': '1'}
    for name, val in re.findall(r'constexpr int (\w+) = (\d+);', src):
        consts.setdefault(name, val)
    out = {}
    for params, name in re.findall(r'template <([^>]*)>[^\n]*\n__global__[^\n]*?void (\w+)\(', src):
        out[name] = [consts.get(p.split('=')[1].strip(), p.split('=')[1].strip()) if '=' in p else None
                     for p in params.split(',')]
    return out, consts


_DEFAULTS, _CONSTS = _template_defaults()


def canon(spelled):
    """'(conv_halo_frag_kernel<3, LU_EPI_LSTM, 4, false>)' -> 'conv_halo_frag_kernel<3, 1, 4, false, 4>'."""
    s = re.sub(r'\s+', ' ', spelled.strip())
    while s.startswith('(') and s.endswith(')'):
        s = s[1:-1].strip()
    m = re.match(r'^(\w+)<(.*)>$', s)
    if not m:
        return s
    name, args = m.group(1), [a.strip() for a in m.group(2).split(',')]
    args = [_CONSTS.get(a, a) for a in args]
    dflt = _DEFAULTS.get(name)
    assert dflt is not None and len(args) <= len(dflt), 'unknown kernel template: ' + s
    args += dflt[len(args):]
    assert None not in args, 'missing template argument: ' + s
    return '%s<%s>' % (name, ', '.join(args))


# ------------------------------------------------------------------------------------------------------------------------
# launch record (emu) and buffers
@pytest.fixture(scope='module', params=BACKENDS)
def be(request):
    return KH.backend(request.param)


class Record(object):
    """Launches of the gated families between start() and stop() (emu); None on the GPU backend."""

    def __init__(self, be):
        self.be = be
        self.lib = None
        if be.name == 'emu':
            self.lib = C.CDLL(be.lib._name)
            self.lib.lu_emu_launches.restype = C.c_size_t
            self.lib.lu_emu_launches.argtypes = [C.c_char_p, C.c_size_t]

    def start(self):
        if self.lib is not None:
            self.lib.lu_emu_launches_reset()

    def stop(self):
        if self.lib is None:
            return None
        n = self.lib.lu_emu_launches(None, 0)
        buf = C.create_string_buffer(n + 1)
        self.lib.lu_emu_launches(buf, n + 1)
        names = [canon(x) for x in buf.value.decode().split('\n') if x]
        return [x for x in names if FAMILY.match(x)]


def dev(be, a, dtype=np.float32):
    d = be.dev(a, dtype)
    assert be.ptr(d) % 16 == 0, 'the harness hands the library 16-byte aligned buffers (the dispatch depends on alignment)'
    return d


def empty(be, shape, dtype=np.float32):
    d = be.empty(shape, dtype)
    assert be.ptr(d) % 16 == 0
    return d


def rnd(rng, *shape, scale=1.0):
    return f32(rng.standard_normal(shape) * scale)


def close(got, ref, tol, what):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max())
    assert np.isfinite(err) and err <= tol, '%s: max |err| %.3e > %.1e' % (what, err, tol)


# ------------------------------------------------------------------------------------------------------------------------
# fp64 references
def conv_ref(x, w, b, stride, dil, pt, pl, Hout, Wout):
    """out[f, oy, ox, n] = b[n] + sum w[kh, kw, c, n] * xd[f, oy*stride + kh - pt, ox*stride + kw - pl, c], xd = x with dil - 1
    zeros between pixels (input dilation), zero outside."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    fr, H, W, Cc = x.shape
    k = w.shape[0]
    Hd, Wd = (H - 1) * dil + 1, (W - 1) * dil + 1
    xd = np.zeros((fr, Hd, Wd, Cc))
    xd[:, ::dil, ::dil] = x
    ph, pw = max(0, (Hout - 1) * stride + k - pt - Hd), max(0, (Wout - 1) * stride + k - pl - Wd)
    xp = np.pad(xd, ((0, 0), (pt, ph), (pl, pw), (0, 0)))
    out = np.zeros((fr, Hout, Wout, w.shape[3]))
    for kh in range(k):
        for kw in range(k):
            patch = xp[:, kh:kh + (Hout - 1) * stride + 1:stride, kw:kw + (Wout - 1) * stride + 1:stride]
            out += np.einsum('fhwc,cn->fhwn', patch, w[kh, kw], optimize=True)
    return out if b is None else out + np.asarray(b, np.float64)


def wgrad_ref(x, dy, k, stride):
    """dw[kh, kw, c, n] = sum x[f, oy*stride + kh - pt, ox*stride + kw - pl, c] * dy[f, oy, ox, n] (TF-SAME padding)."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    _, H, W, Cc = x.shape
    _, Ho, Wo, N = dy.shape
    _, pt, _ = calls.same_pad(H, k, stride)
    _, pl, _ = calls.same_pad(W, k, stride)
    xp = np.pad(x, ((0, 0), (pt, k + (Ho - 1) * stride), (pl, k + (Wo - 1) * stride), (0, 0)))
    dw = np.zeros((k, k, Cc, N))
    for kh in range(k):
        for kw in range(k):
            patch = xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride]
            dw[kh, kw] = np.einsum('fhwc,fhwn->cn', patch, dy, optimize=True)
    return dw


def hard_sigmoid(z):
    return np.clip(0.2 * z + 0.5, 0.0, 1.0)


def lstm_ref(z, c):
    F = c.shape[-1]
    i, f, g, o = (z[..., j * F:(j + 1) * F] for j in range(4))
    c1 = hard_sigmoid(f) * c + hard_sigmoid(i) * np.tanh(g)
    return hard_sigmoid(o) * np.tanh(c1), c1


# ------------------------------------------------------------------------------------------------------------------------
# runners: one descriptor (or a phase-1 / phase-2 pair), the launch record of exactly those calls, the comparison
def run_conv(be, rec, rng, fr, H, W, Cs, N, k, stride=1, dil=1, prec=0, b16=False, splits=1, flags=0, bias=True, post=False,
             out_ps=None, out_rs=0):
    """Cs: channels of each source.  out_ps / out_rs: pixel / row strides of a padded output (canary in the padding)."""
    p = (k - 1) // 2
    if dil == 1:
        Hout, pt, _ = calls.same_pad(H, k, stride)
        Wout, pl, _ = calls.same_pad(W, k, stride)
    else:      # an input-dilated convolution as the stride-`dil` input gradient drives it: full correlation, output = input size
        pt = pl = k - 1 - p
        Hout, Wout = (H - 1) * dil + 1 + 2 * pt - k + 1, (W - 1) * dil + 1 + 2 * pl - k + 1
    xs = [rnd(rng, fr, H, W, c) for c in Cs]
    ws = [rnd(rng, k, k, c, N, scale=2.0 / np.sqrt(k * k * c)) for c in Cs]
    b = rnd(rng, N) if bias else None
    R = bf16_round if prec == 1 else (lambda a: a)
    ref = sum(conv_ref(R(x), R(w), None, stride, dil, pt, pl, Hout, Wout) for x, w in zip(xs, ws))
    if b is not None:
        ref = ref + b
    keep, srcs = [], []
    for x, w in zip(xs, ws):
        c = x.shape[3]
        xd = dev(be, bf16_bits(x), np.int16) if b16 else dev(be, x)
        wd = dev(be, w)
        keep += [xd, wd]
        if prec == 1:
            wd = KH.pack_bf16(be, wd, k, c, N)
            keep.append(wd)
        srcs.append(calls.conv_src(be.ptr(xd), H * W * c, c, c, be.ptr(wd), c * N, N, dtype=cabi.LU_BF16 if b16 else cabi.LU_F32))
    ps = N if out_ps is None else out_ps
    rs = out_rs if out_rs else Wout * ps
    fs = Hout * rs
    out = dev(be, np.full(fr * fs, CANARY, np.uint32).view(np.float32))
    bd = None if b is None else dev(be, b)
    ws_ = empty(be, (splits * fr * Hout * Wout * N + 4,)) if splits > 1 else None
    pd = None
    if post:
        scale, shift = f32(rng.uniform(0.5, 1.5, N)), rnd(rng, N)
        keep += [dev(be, scale), dev(be, shift)]
        pd = (be.ptr(keep[-2]), be.ptr(keep[-1]), 0.3)
        ref = scale * ref + shift
        ref = np.where(ref > 0, ref, 0.3 * ref)
    rec.start()
    calls.conv2d(be.lib, be.stream, srcs, fr, H, W, Hout, Wout, k, stride, dil, pt, pl, N, be.ptr(bd), be.ptr(out), fs, ps,
                 splits=splits, workspace=be.ptr(ws_), out_row_stride=out_rs, precision=prec, flags=flags, post=pd)
    got_rec = rec.stop()
    o = be.host(out)
    full = o.reshape(fr, Hout, rs)
    dense = np.stack([full[:, :, ox * ps:ox * ps + N] for ox in range(Wout)], axis=2)
    close(dense, ref, 5e-5, 'conv')
    mask = np.ones(fr * fs, bool).reshape(fr, Hout, rs)
    for ox in range(Wout):
        mask[:, :, ox * ps:ox * ps + N] = False
    assert np.all(full.view(np.uint32)[mask] == CANARY), 'the padding of a strided output changed'
    return got_rec


def run_lstm(be, rec, rng, fr, H, W, Cin, F, k, prec=0, b16=False, flags=0):
    x, h, c = rnd(rng, fr, H, W, Cin), rnd(rng, fr, H, W, F, scale=0.5), rnd(rng, fr, H, W, F)
    ker, rk, b = rnd(rng, k, k, Cin, 4 * F, scale=0.3), rnd(rng, k, k, F, 4 * F, scale=0.1), rnd(rng, 4 * F, scale=0.5)
    R = bf16_round if prec == 1 else (lambda a: a)
    z = conv_ref(R(x), R(ker), b, 1, 1, (k - 1) // 2, (k - 1) // 2, H, W) + conv_ref(R(h), R(rk), None, 1, 1, (k - 1) // 2,
                                                                                       (k - 1) // 2, H, W)
    h1, c1 = lstm_ref(z, c)
    N = 4 * F
    keep, srcs = [], []
    for t, w, cc in ((x, ker, Cin), (h, rk, F)):
        td = dev(be, bf16_bits(t), np.int16) if b16 else dev(be, t)
        wd = dev(be, w)
        keep += [td, wd]
        if prec == 1:
            wd = KH.pack_bf16(be, wd, k, cc, N)
            keep.append(wd)
        srcs.append(calls.conv_src(be.ptr(td), H * W * cc, cc, cc, be.ptr(wd), cc * N, N, dtype=cabi.LU_BF16 if b16 else cabi.LU_F32))
    cd, bd = dev(be, c), dev(be, b)
    c_out, h_out, gates = empty(be, (fr, H, W, F)), empty(be, (fr, H, W, F)), empty(be, (fr, H, W, N))
    p = (k - 1) // 2
    rec.start()
    calls.conv2d(be.lib, be.stream, srcs, fr, H, W, H, W, k, 1, 1, p, p, N, be.ptr(bd), None, 0, 0,
                 lstm=(be.ptr(cd), H * W * F, be.ptr(c_out), H * W * F, be.ptr(h_out), H * W * F, be.ptr(gates), H * W * N),
                 precision=prec, flags=flags)
    got_rec = rec.stop()
    close(be.host(h_out), h1, 3e-5, 'ConvLSTM h')
    close(be.host(c_out), c1, 3e-5, 'ConvLSTM c')
    return got_rec


def split3(a):
    """Exact three-way bf16 split of fp32 values (lu_split3): hi + mid + lo == a."""
    hi = bf16_round(a)
    r = f32(a - hi)
    mid = bf16_round(r)
    return hi, mid, bf16_round(f32(r - mid))


def run_wgrad(be, rec, rng, fr, H, W, Cc, N, k, stride=1, prec=0, xb=False, yb=False, splits=1, flags=0, beta=0.0, dbias=False,
              dbias_beta=0.0, two_phase=False, dw_ps=None, pieces=False):
    """dw_ps: row stride of a padded dw ([k, k, C, dw_ps], canary in the padding -- the scalar reduce)."""
    Ho, pt, _ = calls.same_pad(H, k, stride)
    Wo, pl, _ = calls.same_pad(W, k, stride)
    x, dy = rnd(rng, fr, H, W, Cc), rnd(rng, fr, Ho, Wo, N, scale=0.5)
    R = bf16_round if prec == 1 else (lambda a: a)
    rs = N if dw_ps is None else dw_ps
    dw0 = np.full((k, k, Cc, rs), CANARY, np.uint32).view(np.float32)
    init = rnd(rng, k, k, Cc, N)
    if beta != 0.0:
        dw0[..., :N] = init
    if pieces:      # split6 operands (x: order A = lo, mid, hi; dy: order B = hi, mid, lo); the kernel sums the six products of ops.SPLIT_TERMS
        px, py = split3(x), split3(dy)
        P = {'hi': 0, 'mid': 1, 'lo': 2}
        terms = (('lo', 'hi'), ('mid', 'mid'), ('hi', 'lo'), ('mid', 'hi'), ('hi', 'mid'), ('hi', 'hi'))
        xs = np.concatenate([px[P[a]] for a, _ in terms], axis=3)      # block t of x against block t of dy is term t
        ys = np.concatenate([py[P[b]] for _, b in terms], axis=3)
        ref = sum(wgrad_ref(px[P[a]], py[P[b]], k, stride) for a, b in terms)
        xd, dyd = dev(be, bf16_bits(xs), np.int16), dev(be, bf16_bits(ys), np.int16)
        d = calls.wgrad_desc(be.ptr(xd), H * W * 6 * Cc, 6 * Cc, Cc, be.ptr(dyd), Ho * Wo * 6 * N, 6 * N, N, fr, H, W, Ho, Wo, k,
                             stride, pt, pl, None, Cc * rs, rs, splits, beta, precision=1, x_dtype=cabi.LU_BF16,
                             dy_dtype=cabi.LU_BF16, flags=flags | cabi.LU_WGRAD_F_PIECES3, terms=6, x_term_stride=Cc,
                             dy_term_stride=N)
        keep = [xd, dyd]
    else:
        ref = wgrad_ref(R(x), R(dy), k, stride)
        xd = dev(be, bf16_bits(x), np.int16) if xb else dev(be, x)
        dyd = dev(be, bf16_bits(dy), np.int16) if yb else dev(be, dy)
        d = calls.wgrad_desc(be.ptr(xd), H * W * Cc, Cc, Cc, be.ptr(dyd), Ho * Wo * N, N, N, fr, H, W, Ho, Wo, k, stride, pt, pl,
                             None, Cc * rs, rs, splits, beta, precision=prec, x_dtype=cabi.LU_BF16 if xb else cabi.LU_F32,
                             dy_dtype=cabi.LU_BF16 if yb else cabi.LU_F32, flags=flags)
        keep = [xd, dyd]
    if beta != 0.0:
        ref = ref + beta * np.asarray(init, np.float64)
    dwd = dev(be, dw0)
    d.dw = be.ptr(dwd)
    db0 = rnd(rng, N)
    dbd = dev(be, db0) if dbias else None
    if dbias:
        d.dbias, d.dbias_beta = be.ptr(dbd), dbias_beta
    ws = empty(be, (be.lib.lu_conv2d_wgrad_workspace_bytes(C.byref(d)) // 4 + 4,))
    d.workspace = be.ptr(ws)
    rec.start()
    for phase in ((1, 2) if two_phase else (0,)):
        d.phase = phase
        calls.check(be.lib, be.lib.lu_conv2d_wgrad(C.byref(d), be.stream), 'wgrad phase %d' % phase)
    got_rec = rec.stop()
    o = be.host(dwd)
    close(o[..., :N], ref, 2e-4, 'wgrad')
    if rs > N:
        assert np.all(o[..., N:].view(np.uint32) == CANARY), 'the padding of a strided dw changed'
    if dbias:
        dsum = np.asarray(bf16_round(dy) if yb else dy, np.float64).reshape(-1, N).sum(0)      # (bf16 dy: the sums of its values)
        close(be.host(dbd), dsum + dbias_beta * np.asarray(db0, np.float64), 2e-4, 'dbias')
    return got_rec


def run_s2(be, rec, rng, kind):
    """The stride-2 bf16 entry points (lu_conv2d_s2_fwd_bf16 / lu_conv2d_s2_dgrad_bf16): even extents."""
    if kind == 'fwd':
        x, w, b = rnd(rng, 2, 6, 10, 40), rnd(rng, 3, 3, 40, 72, scale=0.1), rnd(rng, 72)
        rec.start()
        got = KH.conv2d_s2_fwd_bf16(be, x, w, b)
        r = rec.stop()
        ref = conv_ref(bf16_round(x), bf16_round(w), b, 2, 1, calls.same_pad(6, 3, 2)[1], calls.same_pad(10, 3, 2)[1], 3, 5)
        close(got, ref, 5e-5, 's2 fwd')
        return r
    dy, w = rnd(rng, 2, 3, 5, 64), rnd(rng, 3, 3, 40, 64, scale=0.1)
    rec.start()
    got = KH.conv2d_dgrad_s2_fused_bf16(be, dy, w)
    r = rec.stop()
    # dx = the stride-2 convolution's input gradient: the dy dilated by 2, correlated with the flipped, transposed kernel
    wt = np.ascontiguousarray(np.transpose(w[::-1, ::-1], (0, 1, 3, 2)))
    _, pt, _ = calls.same_pad(6, 3, 2)
    _, pl, _ = calls.same_pad(10, 3, 2)
    ref = conv_ref(bf16_round(dy), bf16_round(wt), None, 1, 2, 2 - pt, 2 - pl, 6, 10)
    close(got, ref, 5e-5, 's2 dgrad')
    return r


# ------------------------------------------------------------------------------------------------------------------------
# the rows: (id, runner, kwargs, expected launch record)
CF = cabi
BIAS, LSTM = 0, 1
HR = 'ksplit_reduce_kernel'
PA = 'post_affine_kernel'
WR = 'wgrad_reduce_kernel'


def conv(id_, exp, **kw):
    return (id_, 'conv', kw, exp)


def lstm(id_, exp, **kw):
    return (id_, 'lstm', kw, exp)


def wg(id_, exp, **kw):
    return (id_, 'wgrad', kw, exp + [WR])


HALO_HW = dict(fr=2, H=15, W=60)      # 8 x 32 patches waste 12 % (<= 25 %: the fp32 halo kernel applies); H % 8, W % 32 != 0
ROWS = [
    # ---- fp32 convolution, LU_EPI_BIAS -------------------------------------------------------------------------------------
    conv('f32_halo3', ['conv_halo_kernel<3, 0, true>'], Cs=[20], N=136, k=3, **HALO_HW),
    conv('f32_halo5_post', ['conv_halo_kernel<5, 0, true>', PA], Cs=[12], N=72, k=5, post=True, **HALO_HW),
    # K split, whole chunks per slice (16-channel chunks: 3 chunks, 3 slices)
    conv('f32_halo3_split_chunks', ['conv_halo_kernel<3, 0, true>', HR], Cs=[40], N=132, k=3, splits=3, **HALO_HW),
    # K split, counted loop (2 chunks, 3 slices: a slice starts inside a chunk)
    conv('f32_halo3_split_counted', ['conv_halo_kernel<3, 0, false>', HR], Cs=[20], N=136, k=3, splits=3, **HALO_HW),
    conv('f32_halo5_split_counted', ['conv_halo_kernel<5, 0, false>', HR], Cs=[12, 8], N=72, k=5, splits=3, **HALO_HW),
    # general kernel: 8 x 32 patches of a 9 x 7 image waste far more than 25 % (not the halo kernel)
    conv('f32_gen_nf4_wide', ['conv_fwd_kernel<4, true, 0, false, 1, false>'], fr=2, H=9, W=7, Cs=[20], N=136, k=3),
    conv('f32_gen_nf4_scalar', ['conv_fwd_kernel<4, false, 0, false, 2, false>'], fr=2, H=9, W=7, Cs=[8], N=70, k=3),
    conv('f32_gen_nf2', ['conv_fwd_kernel<2, true, 0, false, 2, false>'], fr=2, H=9, W=7, Cs=[20], N=40, k=3, stride=2),
    conv('f32_gen_nf2_scalar', ['conv_fwd_kernel<2, false, 0, false, 2, false>'], fr=2, H=9, W=7, Cs=[8], N=38, k=5),
    conv('f32_gen_nf1', ['conv_fwd_kernel<1, true, 0, false, 2, false>'], fr=2, H=9, W=7, Cs=[3, 8], N=12, k=3),
    conv('f32_gen_nf1_scalar', ['conv_fwd_kernel<1, false, 0, false, 2, false>'], fr=2, H=9, W=7, Cs=[8], N=3, k=1),
    # strided output (pixel AND row stride, canary in the padding) through the K-split reduce
    conv('f32_gen_strided_split', ['conv_fwd_kernel<4, true, 0, false, 1, false>', HR], fr=2, H=9, W=7, Cs=[24], N=72, k=3,
         splits=2, out_ps=76, out_rs=7 * 76 + 8),
    # input dilation (the stride-2 input gradient): the fully general instantiation, one per column-fragment count / weight form
    conv('f32_dil_nf4', ['conv_fwd_kernel<4, true, 0, true, 2, false>'], fr=2, H=5, W=4, Cs=[8], N=72, k=3, dil=2),
    conv('f32_dil_nf4_scalar', ['conv_fwd_kernel<4, false, 0, true, 2, false>'], fr=2, H=5, W=4, Cs=[8], N=66, k=3, dil=2),
    conv('f32_dil_nf2', ['conv_fwd_kernel<2, true, 0, true, 2, false>'], fr=2, H=5, W=4, Cs=[12], N=40, k=3, dil=2),
    conv('f32_dil_nf2_scalar', ['conv_fwd_kernel<2, false, 0, true, 2, false>'], fr=2, H=5, W=4, Cs=[8], N=34, k=3, dil=2),
    conv('f32_dil_nf1', ['conv_fwd_kernel<1, true, 0, true, 2, false>'], fr=2, H=5, W=4, Cs=[12], N=20, k=5, dil=2),
    conv('f32_dil_nf1_scalar', ['conv_fwd_kernel<1, false, 0, true, 2, false>'], fr=2, H=5, W=4, Cs=[8], N=7, k=3, dil=2),
    # ---- fp32 ConvLSTM step (fused gate epilogue) ---------------------------------------------------------------------------
    lstm('f32_lstm_halo3', ['conv_halo_kernel<3, 1, true>'], Cin=12, F=32, k=3, **HALO_HW),
    lstm('f32_lstm_halo5', ['conv_halo_kernel<5, 1, true>'], Cin=12, F=32, k=5, **HALO_HW),
    lstm('f32_lstm_general', ['conv_fwd_kernel<4, true, 1, false, 1, false>'], fr=2, H=6, W=7, Cin=12, F=32, k=3),
    # ---- bf16 convolution (precision 1) --------------------------------------------------------------------------------------
    conv('bf16_narrow3_n32', ['conv_halo_frag_kernel<3, 0, 1, false, 1>'], fr=2, H=11, W=40, Cs=[40], N=32, k=3, prec=1),
    conv('bf16_narrow3_n32_b16', ['conv_halo_frag_kernel<3, 0, 1, true, 1>'], fr=2, H=11, W=40, Cs=[40], N=32, k=3, prec=1, b16=True),
    conv('bf16_narrow5_n32', ['conv_halo_frag_kernel<5, 0, 1, false, 1>'], fr=2, H=11, W=40, Cs=[40], N=32, k=5, prec=1),
    conv('bf16_narrow5_n32_b16', ['conv_halo_frag_kernel<5, 0, 1, true, 1>'], fr=2, H=11, W=40, Cs=[40], N=32, k=5, prec=1, b16=True),
    conv('bf16_narrow3_n64', ['conv_halo_frag_kernel<3, 0, 2, false, 2>'], fr=2, H=11, W=40, Cs=[40], N=64, k=3, prec=1),
    conv('bf16_narrow3_n64_b16', ['conv_halo_frag_kernel<3, 0, 2, true, 2>'], fr=2, H=11, W=40, Cs=[40], N=64, k=3, prec=1, b16=True),
    conv('bf16_narrow5_n64', ['conv_halo_frag_kernel<5, 0, 2, false, 2>'], fr=2, H=11, W=40, Cs=[40], N=64, k=5, prec=1),
    # narrow block with a K split and a padded pixel stride (canary)
    conv('bf16_narrow5_n64_b16_split', ['conv_halo_frag_kernel<5, 0, 2, true, 2>', HR], fr=2, H=11, W=40, Cs=[40], N=64, k=5,
         prec=1, b16=True, splits=2, out_ps=68),
    conv('bf16_halo3', ['conv_halo_frag_kernel<3, 0, 4, false, 4>'], fr=2, H=11, W=40, Cs=[40], N=136, k=3, prec=1),
    conv('bf16_halo3_b16_split', ['conv_halo_frag_kernel<3, 0, 4, true, 4>', HR], fr=2, H=11, W=40, Cs=[40, 16], N=136, k=3,
         prec=1, b16=True, splits=2),
    conv('bf16_halo5', ['conv_halo_frag3_kernel<5, 0, 4, false, 2>'], fr=2, H=11, W=40, Cs=[40], N=72, k=5, prec=1),
    conv('bf16_halo5_b16_post', ['conv_halo_frag3_kernel<5, 0, 4, true, 2>', PA], fr=2, H=11, W=40, Cs=[40], N=136, k=5, prec=1,
         b16=True, post=True),
    # 16-row patches: the library's own choice from >= 256 blocks on; forced (LU_CONV_F_PATCH16) at emulator sizes
    conv('bf16_halo5_p16', ['conv_halo_frag3_kernel<5, 0, 8, false, 2>'], fr=2, H=19, W=40, Cs=[40], N=72, k=5, prec=1,
         flags=CF.LU_CONV_F_PATCH16),
    conv('bf16_halo5_p16_b16', ['conv_halo_frag3_kernel<5, 0, 8, true, 2>'], fr=2, H=19, W=40, Cs=[40], N=72, k=5, prec=1,
         b16=True, flags=CF.LU_CONV_F_PATCH16),
    conv('bf16_halo3_p16_b16', ['conv_halo_frag3_kernel<3, 0, 8, true, 2>'], fr=2, H=19, W=40, Cs=[40], N=72, k=3, prec=1,
         b16=True, flags=CF.LU_CONV_F_PATCH16),
    # half blocks: the library's own choice from >= 512 blocks on; forced (LU_CONV_F_HALF_BLOCK) at emulator sizes
    conv('bf16_half5', ['conv_halo_frag3_kernel<5, 0, 8, false, 1>'], fr=2, H=11, W=40, Cs=[40], N=72, k=5, prec=1,
         flags=CF.LU_CONV_F_HALF_BLOCK),
    conv('bf16_half5_b16', ['conv_halo_frag3_kernel<5, 0, 8, true, 1>'], fr=2, H=11, W=40, Cs=[40], N=72, k=5, prec=1, b16=True,
         flags=CF.LU_CONV_F_HALF_BLOCK),
    conv('bf16_half3_b16', ['conv_halo_frag3_kernel<3, 0, 8, true, 1>'], fr=2, H=11, W=40, Cs=[40], N=136, k=3, prec=1, b16=True,
         flags=CF.LU_CONV_F_HALF_BLOCK),
    conv('bf16_gather_s2', ['conv_gather_bf16_kernel'], fr=2, H=11, W=13, Cs=[40], N=72, k=3, stride=2, prec=1),
    # ---- bf16 ConvLSTM step --------------------------------------------------------------------------------------------------
    lstm('bf16_lstm3', ['conv_halo_frag_kernel<3, 1, 4, false, 4>'], fr=2, H=11, W=40, Cin=8, F=32, k=3, prec=1),
    lstm('bf16_lstm3_b16', ['conv_halo_frag_kernel<3, 1, 4, true, 4>'], fr=2, H=11, W=40, Cin=8, F=32, k=3, prec=1, b16=True),
    lstm('bf16_lstm5', ['conv_halo_frag3_kernel<5, 1, 4, false, 2>'], fr=2, H=11, W=40, Cin=8, F=32, k=5, prec=1),
    lstm('bf16_lstm5_b16', ['conv_halo_frag3_kernel<5, 1, 4, true, 2>'], fr=2, H=11, W=40, Cin=8, F=32, k=5, prec=1, b16=True),
    lstm('bf16_lstm5_p16', ['conv_halo_frag3_kernel<5, 1, 8, false, 2>'], fr=2, H=19, W=40, Cin=8, F=32, k=5, prec=1,
         flags=CF.LU_CONV_F_PATCH16),
    lstm('bf16_lstm5_p16_b16', ['conv_halo_frag3_kernel<5, 1, 8, true, 2>'], fr=2, H=19, W=40, Cin=8, F=32, k=5, prec=1, b16=True,
         flags=CF.LU_CONV_F_PATCH16),
    lstm('bf16_lstm5_half', ['conv_halo_frag3_kernel<5, 1, 8, false, 1>'], fr=2, H=11, W=40, Cin=8, F=32, k=5, prec=1,
         flags=CF.LU_CONV_F_HALF_BLOCK),
    lstm('bf16_lstm5_half_b16', ['conv_halo_frag3_kernel<5, 1, 8, true, 1>'], fr=2, H=11, W=40, Cin=8, F=32, k=5, prec=1, b16=True,
         flags=CF.LU_CONV_F_HALF_BLOCK),
    lstm('bf16_lstm3_half_b16', ['conv_halo_frag3_kernel<3, 1, 8, true, 1>'], fr=2, H=11, W=40, Cin=8, F=32, k=3, prec=1, b16=True,
         flags=CF.LU_CONV_F_HALF_BLOCK),
    # ---- stride-2 bf16 entry points ------------------------------------------------------------------------------------------
    ('bf16_s2_fwd', 's2', {'kind': 'fwd'}, ['conv_s2_fwd_bf16_kernel']),
    ('bf16_s2_dgrad', 's2', {'kind': 'dgrad'}, ['conv_s2_dgrad_bf16_kernel']),
    # ---- fp32 weight gradient ------------------------------------------------------------------------------------------------
    # general kernel (W = 7: neither kernel-row nor all-taps form)
    wg('f32_wg_thin', ['wgrad_kernel<1, 1, 1, 4, true, true>'], fr=2, H=5, W=7, Cc=6, N=12, k=3),
    wg('f32_wg_thin_scalar', ['wgrad_kernel<1, 1, 1, 4, true, false>'], fr=2, H=5, W=7, Cc=6, N=10, k=3, splits=2),
    # tiny reduce: slab 9 * 8 * 12 <= 16384 elements, 64 splits (parallel over the slabs as well); 4080 pixels = 64 slabs of 64 with a
    # short last one: every slab holds data
    wg('f32_wg_c32_tiny', ['wgrad_kernel<1, 1, 1, 4, false, true>'], fr=2, H=34, W=60, Cc=8, N=12, k=3, splits=64),
    wg('f32_wg_c32_scalar', ['wgrad_kernel<1, 1, 1, 4, false, false>'], fr=2, H=5, W=7, Cc=20, N=10, k=3),
    wg('f32_wg_c64', ['wgrad_kernel<2, 1, 1, 4, false, true>'], fr=2, H=5, W=7, Cc=40, N=20, k=3, beta=0.5),
    wg('f32_wg_c64_scalar', ['wgrad_kernel<2, 1, 1, 4, false, false>'], fr=2, H=5, W=7, Cc=40, N=18, k=5),
    wg('f32_wg_wide', ['wgrad_kernel<2, 2, 2, 2, false, true>'], fr=2, H=5, W=7, Cc=72, N=40, k=3, splits=2),
    wg('f32_wg_wide_scalar', ['wgrad_kernel<2, 2, 2, 2, false, false>'], fr=2, H=5, W=7, Cc=72, N=42, k=3),
    wg('f32_wg_wide_n256', ['wgrad_kernel<2, 4, 2, 2, false, true>'], fr=2, H=3, W=7, Cc=72, N=264, k=3, splits=2),
    # all-taps 3x3 form (C, N <= 64, W % 16 == 0) with 2 / 3 / 5 accumulator tiles per wave
    wg('f32_small3_t2', ['wgrad_small3_kernel<2>'], fr=2, H=5, W=16, Cc=20, N=24, k=3, dbias=True, dbias_beta=1.0),
    wg('f32_small3_t3', ['wgrad_small3_kernel<3>'], fr=2, H=5, W=16, Cc=40, N=24, k=3, splits=2),
    wg('f32_small3_t5', ['wgrad_small3_kernel<5>'], fr=2, H=5, W=16, Cc=40, N=36, k=3, beta=1.0),
    # kernel-row form (C >= 64): ragged widths (W % 16 != 0, W >= 40), 16- and 32-pixel stages
    wg('f32_row3_ragged', ['wgrad_row_kernel<3, true, 16>'], fr=2, H=3, W=40, Cc=72, N=40, k=3, splits=3, dbias=True,
       dbias_beta=0.5),
    wg('f32_row5_ragged', ['wgrad_row_kernel<5, true, 16>'], fr=2, H=3, W=44, Cc=72, N=40, k=5, splits=2),
    wg('f32_row3_p16', ['wgrad_row_kernel<3, false, 16>'], fr=2, H=3, W=48, Cc=72, N=40, k=3, beta=1.0),
    wg('f32_row5_p16', ['wgrad_row_kernel<5, false, 16>'], fr=2, H=3, W=16, Cc=72, N=40, k=5, two_phase=True),
    wg('f32_row3_p32', ['wgrad_row_kernel<3, false, 32>'], fr=2, H=3, W=32, Cc=72, N=40, k=3, splits=2),
    # scalar reduce: dw rows padded to 43 floats (no 16-byte groups), canary in the padding
    wg('f32_row5_p32_scalar_reduce', ['wgrad_row_kernel<5, false, 32>'], fr=2, H=3, W=32, Cc=72, N=40, k=5, dw_ps=43, beta=0.5),
    # ---- bf16 weight gradient (precision 1; W % 32 == 0 throughout) --------------------------------------------------------------
    # 1x1 (im2col chunk of a thin input, C >= 32), every operand mix
    wg('bf16_k1_ff', ['wgrad_row_bf16_kernel<1, 64, false, false, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=40, N=40, k=1, prec=1),
    wg('bf16_k1_fb', ['wgrad_row_bf16_kernel<1, 64, false, true, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=40, N=40, k=1, prec=1,
       yb=True),
    wg('bf16_k1_bf', ['wgrad_row_bf16_kernel<1, 64, true, false, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=40, N=40, k=1, prec=1,
       xb=True, splits=2),
    wg('bf16_k1_bb', ['wgrad_row_bf16_kernel<1, 64, true, true, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=40, N=40, k=1, prec=1,
       xb=True, yb=True, beta=1.0),
    # stride 2, 5x5 (64-channel tiles), every operand mix
    wg('bf16_s2k5_ff', ['wgrad_row_bf16_kernel<5, 64, false, false, 2, 32, 1, 8, false>'], fr=2, H=5, W=64, Cc=72, N=40, k=5,
       stride=2, prec=1),
    wg('bf16_s2k5_fb', ['wgrad_row_bf16_kernel<5, 64, false, true, 2, 32, 1, 8, false>'], fr=2, H=5, W=64, Cc=72, N=40, k=5,
       stride=2, prec=1, yb=True),
    wg('bf16_s2k5_bf', ['wgrad_row_bf16_kernel<5, 64, true, false, 2, 32, 1, 8, false>'], fr=2, H=5, W=64, Cc=72, N=40, k=5,
       stride=2, prec=1, xb=True, dbias=True, dbias_beta=1.0),
    wg('bf16_s2k5_bb', ['wgrad_row_bf16_kernel<5, 64, true, true, 2, 32, 1, 8, false>'], fr=2, H=5, W=64, Cc=72, N=40, k=5,
       stride=2, prec=1, xb=True, yb=True),
    # stride 2, 3x3, 64-channel tiles
    wg('bf16_s2k3_ff', ['wgrad_row_bf16_kernel<3, 64, false, false, 2, 32, 1, 8, false>'], fr=2, H=5, W=64, Cc=72, N=40, k=3,
       stride=2, prec=1),
    wg('bf16_s2k3_fb', ['wgrad_row_bf16_kernel<3, 64, false, true, 2, 32, 1, 8, false>'], fr=2, H=5, W=64, Cc=72, N=40, k=3,
       stride=2, prec=1, yb=True),
    wg('bf16_s2k3_bf', ['wgrad_row_bf16_kernel<3, 64, true, false, 2, 32, 1, 8, false>'], fr=2, H=5, W=64, Cc=72, N=40, k=3,
       stride=2, prec=1, xb=True),
    wg('bf16_s2k3_bb', ['wgrad_row_bf16_kernel<3, 64, true, true, 2, 32, 1, 8, false>'], fr=2, H=5, W=64, Cc=72, N=40, k=3,
       stride=2, prec=1, xb=True, yb=True, splits=2),
    # stride 2, 3x3, 128-channel tiles (C % 128 == 0)
    wg('bf16_s2k3_c128_ff', ['wgrad_row_bf16_kernel<3, 128, false, false, 2, 32, 1, 8, false>'], fr=2, H=3, W=64, Cc=128, N=40, k=3,
       stride=2, prec=1),
    wg('bf16_s2k3_c128_fb', ['wgrad_row_bf16_kernel<3, 128, false, true, 2, 32, 1, 8, false>'], fr=2, H=3, W=64, Cc=128, N=40, k=3,
       stride=2, prec=1, yb=True),
    wg('bf16_s2k3_c128_bf', ['wgrad_row_bf16_kernel<3, 128, true, false, 2, 32, 1, 8, false>'], fr=2, H=3, W=64, Cc=128, N=40, k=3,
       stride=2, prec=1, xb=True),
    wg('bf16_s2k3_c128_bb', ['wgrad_row_bf16_kernel<3, 128, true, true, 2, 32, 1, 8, false>'], fr=2, H=3, W=64, Cc=128, N=40, k=3,
       stride=2, prec=1, xb=True, yb=True),
    # stride 1, 5x5, 64-channel tiles
    wg('bf16_k5_c64_ff', ['wgrad_row_bf16_kernel<5, 64, false, false, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=5,
       prec=1),
    wg('bf16_k5_c64_fb', ['wgrad_row_bf16_kernel<5, 64, false, true, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=5,
       prec=1, yb=True),
    wg('bf16_k5_c64_bf', ['wgrad_row_bf16_kernel<5, 64, true, false, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=5,
       prec=1, xb=True),
    wg('bf16_k5_c64_bb', ['wgrad_row_bf16_kernel<5, 64, true, true, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=5,
       prec=1, xb=True, yb=True, dbias=True, dbias_beta=0.0),
    # stride 1, 5x5, 128-channel tiles: the library's choice for C % 128 == 0 or C > 256; forced (LU_WGRAD_F_CT128) to give a masked
    # channel tail at an emulator size.  32-pixel stages (W % 64 != 0) ...
    wg('bf16_k5_c128_ff', ['wgrad_row_bf16_kernel<5, 128, false, false, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=5,
       prec=1, flags=CF.LU_WGRAD_F_CT128),
    wg('bf16_k5_c128_fb', ['wgrad_row_bf16_kernel<5, 128, false, true, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=5,
       prec=1, yb=True, flags=CF.LU_WGRAD_F_CT128),
    wg('bf16_k5_c128_bf', ['wgrad_row_bf16_kernel<5, 128, true, false, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=5,
       prec=1, xb=True, flags=CF.LU_WGRAD_F_CT128, splits=2),
    wg('bf16_k5_c128_bb', ['wgrad_row_bf16_kernel<5, 128, true, true, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=128, N=40, k=5,
       prec=1, xb=True, yb=True),
    # ... and 64-pixel stages (W % 64 == 0)
    wg('bf16_k5_c128_p64_ff', ['wgrad_row_bf16_kernel<5, 128, false, false, 1, 64, 1, 8, false>'], fr=2, H=2, W=64, Cc=72, N=40,
       k=5, prec=1, flags=CF.LU_WGRAD_F_CT128),
    wg('bf16_k5_c128_p64_fb', ['wgrad_row_bf16_kernel<5, 128, false, true, 1, 64, 1, 8, false>'], fr=2, H=2, W=64, Cc=72, N=40,
       k=5, prec=1, yb=True, flags=CF.LU_WGRAD_F_CT128),
    wg('bf16_k5_c128_p64_bf', ['wgrad_row_bf16_kernel<5, 128, true, false, 1, 64, 1, 8, false>'], fr=2, H=2, W=64, Cc=72, N=40,
       k=5, prec=1, xb=True, flags=CF.LU_WGRAD_F_CT128),
    wg('bf16_k5_c128_p64_bb', ['wgrad_row_bf16_kernel<5, 128, true, true, 1, 64, 1, 8, false>'], fr=2, H=2, W=64, Cc=128, N=40,
       k=5, prec=1, xb=True, yb=True, two_phase=True, splits=2),
    # stride 1, 3x3, kernel-row form: 64-channel tiles for 32 <= C < 64 (the all-taps form needs C >= 64) ...
    wg('bf16_k3_c64_ff', ['wgrad_row_bf16_kernel<3, 64, false, false, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=40, N=40, k=3,
       prec=1),
    wg('bf16_k3_c64_fb', ['wgrad_row_bf16_kernel<3, 64, false, true, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=40, N=40, k=3,
       prec=1, yb=True),
    wg('bf16_k3_c64_bf', ['wgrad_row_bf16_kernel<3, 64, true, false, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=40, N=40, k=3,
       prec=1, xb=True),
    wg('bf16_k3_c64_bb', ['wgrad_row_bf16_kernel<3, 64, true, true, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=40, N=40, k=3,
       prec=1, xb=True, yb=True),
    # ... 128-channel tiles: only by flag (LU_WGRAD_F_CT128; without it a C that takes 128-channel tiles takes the all-taps form)
    wg('bf16_k3_c128_ff', ['wgrad_row_bf16_kernel<3, 128, false, false, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=3,
       prec=1, flags=CF.LU_WGRAD_F_CT128),
    wg('bf16_k3_c128_fb', ['wgrad_row_bf16_kernel<3, 128, false, true, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=3,
       prec=1, yb=True, flags=CF.LU_WGRAD_F_CT128),
    wg('bf16_k3_c128_bf', ['wgrad_row_bf16_kernel<3, 128, true, false, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=3,
       prec=1, xb=True, flags=CF.LU_WGRAD_F_CT128),
    wg('bf16_k3_c128_bb', ['wgrad_row_bf16_kernel<3, 128, true, true, 1, 32, 1, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=3,
       prec=1, xb=True, yb=True, flags=CF.LU_WGRAD_F_CT128),
    # stride 1, 3x3, all-taps form (C >= 64): register staging for mixed operands ...
    wg('bf16_taps9_ff', ['wgrad_row_bf16_kernel<3, 64, false, false, 1, 32, 3, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=3,
       prec=1),
    wg('bf16_taps9_fb', ['wgrad_row_bf16_kernel<3, 64, false, true, 1, 32, 3, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=3,
       prec=1, yb=True),
    wg('bf16_taps9_bf', ['wgrad_row_bf16_kernel<3, 64, true, false, 1, 32, 3, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=3,
       prec=1, xb=True, dbias=True, dbias_beta=1.0),
    # ... bf16 operands: LDS-DMA staging (the library's choice) with 32- and 64-pixel stages; register staging only by flag
    # (LU_WGRAD_F_NO_DMA)
    wg('bf16_taps9_bb_dma', ['wgrad_row_bf16_kernel<3, 64, true, true, 1, 32, 3, 8, true>'], fr=2, H=3, W=32, Cc=72, N=40, k=3,
       prec=1, xb=True, yb=True, splits=2),
    wg('bf16_taps9_bb_dma_p64', ['wgrad_row_bf16_kernel<3, 64, true, true, 1, 64, 3, 8, true>'], fr=2, H=2, W=64, Cc=72, N=40, k=3,
       prec=1, xb=True, yb=True),
    wg('bf16_taps9_bb_regs', ['wgrad_row_bf16_kernel<3, 64, true, true, 1, 32, 3, 8, false>'], fr=2, H=3, W=32, Cc=72, N=40, k=3,
       prec=1, xb=True, yb=True, flags=CF.LU_WGRAD_F_NO_DMA),
    wg('bf16_taps9_bb_regs_p64', ['wgrad_row_bf16_kernel<3, 64, true, true, 1, 64, 3, 8, false>'], fr=2, H=2, W=64, Cc=72, N=40,
       k=3, prec=1, xb=True, yb=True, flags=CF.LU_WGRAD_F_NO_DMA),
    # piece-aware 'bf16x3' kernel (split6 operands, C % 128 == 0)
    wg('x3_pieces3', ['wgrad_row_x3_kernel<3>'], fr=2, H=2, W=32, Cc=128, N=40, k=3, pieces=True, dbias=True, dbias_beta=1.0),
    wg('x3_pieces5', ['wgrad_row_x3_kernel<5>'], fr=1, H=2, W=32, Cc=128, N=40, k=5, pieces=True, splits=2),
]
ROW_IDS = [r[0] for r in ROWS]
assert len(set(ROW_IDS)) == len(ROW_IDS)
RUNNERS = {'conv': run_conv, 'lstm': run_lstm, 'wgrad': run_wgrad, 's2': run_s2}


def _expected(row):
    return [canon(x) for x in row[3]]


@pytest.mark.parametrize('row', ROWS, ids=ROW_IDS)
def test_dispatch_row(be, row):
    """The row's descriptor reaches the row's instance(s) (emu: the launch record, in order) and matches the fp64 reference."""
    id_, kind, kw, _ = row
    rng = np.random.default_rng(zlib.crc32(id_.encode()))
    got = RUNNERS[kind](be, Record(be), rng, **kw)
    if got is not None:
        assert got == _expected(row), '%s reached %s, expected %s' % (id_, got, _expected(row))


# ------------------------------------------------------------------------------------------------------------------------
# the coverage gate (CPU)
def _golden():
    with open(GOLDEN) as fh:
        return sorted(l.strip() for l in fh if l.strip() and not l.startswith('#'))


# compiled, but no descriptor reaches them through the C ABI (kept out of the rows, listed here so that the gate stays exact)
UNREACHABLE = {
    'conv_fwd_kernel<4, true, 0, false, 2, false>': 'LU_CONV_CASE(4, true) in lu_conv2d_fwd: the branch before it (NF_ == 4 && BV_) '
                                                    'takes every such launch to conv_fwd_kernel<4, true, 0, false, 1, false>',
}


def test_every_instance_has_a_row():
    covered = set(x for r in ROWS for x in _expected(r))
    golden = set(_golden())
    assert set(UNREACHABLE) <= golden and not covered & set(UNREACHABLE), 'stale UNREACHABLE entry'
    covered |= set(UNREACHABLE)
    assert not golden - covered, 'instances without a dispatch row: %s' % sorted(golden - covered)
    assert not covered - golden, 'rows expect instances missing from %s: %s' % (os.path.basename(GOLDEN), sorted(covered - golden))


def code_object_instances(lib_path):
    """Gated kernel symbols of the gfx950 code objects bundled in the library (one bundle per translation unit)."""
    llvm = '/opt/rocm/lib/llvm/bin'
    tools = {t: (os.path.join(llvm, t) if os.path.exists(os.path.join(llvm, t)) else shutil.which(t))
             for t in ('llvm-objcopy', 'clang-offload-bundler', 'llvm-readelf')}
    missing = [t for t, p in tools.items() if not p]
    if missing:
        pytest.skip('ROCm LLVM tools not found: %s' % ', '.join(missing))
    names = set()
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, 'fat.bin')
        subprocess.check_call([tools['llvm-objcopy'], '--dump-section=.hip_fatbin=' + fat, lib_path, os.path.join(tmp, 'lib.so')])
        data = open(fat, 'rb').read()
        starts = [m.start() for m in re.finditer(b'__CLANG_OFFLOAD_BUNDLE__', data)]
        assert starts, 'no offload bundle in ' + lib_path
        for i, s in enumerate(starts):
            part, co = os.path.join(tmp, 'b%d.bin' % i), os.path.join(tmp, 'co%d.o' % i)
            with open(part, 'wb') as fh:
                fh.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
            subprocess.check_call([tools['clang-offload-bundler'], '--unbundle', '--type=o', '--input=' + part,
                                   '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + co])
            out = subprocess.check_output([tools['llvm-readelf'], '-sW', '--demangle', co]).decode()
            for line in out.splitlines():
                f = line.split(None, 7)
                if len(f) == 8 and f[3] == 'FUNC' and f[4] == 'GLOBAL':
                    n = re.sub(r'\(anonymous namespace\)::', '', f[7])
                    n = re.sub(r'^void ', '', n)
                    n = re.sub(r'\([^()]*\)$', '', n).strip()
                    if FAMILY.match(n):
                        names.add(canon(n))
    return names


def test_instance_list_matches_the_code_object():
    from lu_native import build as B
    if B.needs_build():
        pytest.skip('the gfx950 library is not built from these sources (run __graft_entry__.build())')
    found = code_object_instances(B.LIB)
    golden = set(_golden())
    assert not found - golden, 'compiled instances missing from %s: %s' % (os.path.basename(GOLDEN), sorted(found - golden))
    assert not golden - found, 'listed instances not in the code object: %s' % sorted(golden - found)


def test_canonical_names():
    assert canon('(conv_halo_frag_kernel<3, LU_EPI_LSTM, 4, false>)') == 'conv_halo_frag_kernel<3, 1, 4, false, 4>'
    assert canon('(wgrad_row_bf16_kernel<5, 128, true, false, 1, 64>)') == \
        'wgrad_row_bf16_kernel<5, 128, true, false, 1, 64, 1, 8, false>'
    assert canon('(conv_halo_kernel<3,  LU_EPI_BIAS>)') == 'conv_halo_kernel<3, 0, false>'
    assert canon('wgrad_reduce_kernel') == 'wgrad_reduce_kernel'
