"""Thin Python wrappers over the C ABI (include/dam_hip.h): shape checks, output allocation through
torch's caching allocator, launch on the current torch stream.  No arithmetic happens here and
there is no CPU fallback."""
import collections
import ctypes
import numbers
import os

import torch

from . import _lib


def _f32c(t, name):
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError('%s must be a contiguous float32 tensor' % name)
    return t


def conv_out_size(n, k, stride=1, pad=0, dil=1):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


# ----------------------------------------------------------------------------- convolution
def pack_weights(w, transpose=False, out=None):
    """[O,I,KH,KW] -> packed image for the forward (transpose=False) or dgrad operator."""
    _lib.require_cuda(w)
    w = _f32c(w.detach(), 'weight')
    o, i, kh, kw = w.shape
    n_out, k_in = (i, o) if transpose else (o, i)
    n = _lib.lib().dam_conv_packed_weight_count(n_out, k_in, kh, kw)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=w.device)
    _lib.check(_lib.lib().dam_conv_pack_weights_f32(_lib.ptr(w), o, i, kh, kw, 1 if transpose else 0,
                                                    _lib.ptr(out), _lib.stream()), 'dam_conv_pack_weights_f32')
    return out


def pack_weights_multi(desc, n_tensors, max_total):
    """desc: CUDA int64 tensor [n,8] = {src ptr, dst ptr, O, I, KH, KW, transpose, count}: all packs in one launch."""
    _lib.check(_lib.lib().dam_conv_pack_weights_multi_f32(_lib.ptr(desc), n_tensors, max_total, _lib.stream()),
               'dam_conv_pack_weights_multi_f32')


# strided 3x3 data gradients of the thin stages as one launch (dam_dgrad_s2_3x3_f32); DAM_NO_DGRAD_S2=1: the parity-class launches (A/B)
DGRAD_S2 = not os.environ.get('DAM_NO_DGRAD_S2')
dgrad_s2_launches = 0        # launches dam_dgrad_s2_3x3_f32 accepted (tests check that a shape took the one-launch form)
# BatchNorm-backward sums from the data-gradient epilogue (include/dam_hip.h: dam_bn_bwd_sums); DAM_NO_DGRAD_SUMS=1 keeps the
# separate pass over dy and x (A/B switch)
DGRAD_BN_SUMS = not os.environ.get('DAM_NO_DGRAD_SUMS')


def _bn_fin_struct(bn, out4):
    """bn = (gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps); out4: [4, C] result rows."""
    gamma, beta, rm, rv, nbt, mom, eps = bn
    return _lib.BnFin(_lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(nbt), float(mom), float(eps),
                      _lib.ptr(out4[0]), _lib.ptr(out4[1]), _lib.ptr(out4[2]), _lib.ptr(out4[3]))


# The scalar arguments of dam_conv2d_tapgrid_f32 / dam_conv2d_tapgrid_plan (all but relu_in / relu_out), in the header's order
TapGrid = collections.namedtuple('TapGrid', 'B H W C in_nchw k_chunks n_out OHt OWt Ho Wo out_stride oo_h oo_w in_stride nA nB '
                                            'off_h step_h off_w step_w wt_base wt_sa wt_sb')
# dam_conv2d_tapgrid_plan's `operands` bits (include/dam_hip.h: DAM_CONV_HAS_*)
_HAS = dict(bias=0x001, in_scale=0x002, in_shift=0x004, res=0x008, res_mask=0x010, bn_partial=0x020, bn_bwd=0x040,
            bwd_mask_bits=0x080, bwd_res_mask_bits=0x100, bwd_mask_scale=0x200, workspace=0x400, batch=0x800, bn_in=0x1000,
            bn_in_bits=0x2000)


def _given(v):
    """An optional operand of a plan call: a tensor or True stands for "given", None or False for "absent"."""
    return v is not None and v is not False


def _fwd_grid(x_shape, n_out, kh, kw, stride, pad, dil, in_nchw):
    """Tap grid of a forward convolution of an input of x_shape (NHWC, or NCHW if in_nchw)."""
    if in_nchw:
        B, C, H, W = x_shape
        k_chunks = 1
    else:
        B, H, W, C = x_shape
        k_chunks = C // 16
    Ho, Wo = conv_out_size(H, kh, stride, pad, dil), conv_out_size(W, kw, stride, pad, dil)
    if Ho <= 0 or Wo <= 0:
        raise ValueError('convolution output would be empty')
    return TapGrid(B, H, W, C, 1 if in_nchw else 0, k_chunks, (n_out + 15) // 16 * 16, Ho, Wo, Ho, Wo, 1, 0, 0, stride, kh, kw,
                   -pad, dil, -pad, dil, 0, kw, 1)


def _dgrad_grid(dy_shape, n_in, H, W, kh, kw, stride, pad, dil, ph=0, pw=0):
    """Tap grid of the data gradient [B, H, W, n_in16] of a convolution with output dy_shape, output parity class (ph, pw) -- the
    whole gradient at stride 1; None for a class that has no pixels or receives no taps."""
    B, Ho, Wo, Co = dy_shape
    ah, aw = _dgrad_axis(ph, pad, dil, kh, stride), _dgrad_axis(pw, pad, dil, kw, stride)
    nh, nw = (H - ph + stride - 1) // stride, (W - pw + stride - 1) // stride
    if nh <= 0 or nw <= 0 or ah is None or aw is None:
        return None
    return TapGrid(B, Ho, Wo, Co, 0, Co // 16, (n_in + 15) // 16 * 16, H, W, nh, nw, stride, ph, pw, 1, ah[0], aw[0],
                   ah[3], ah[4], aw[3], aw[4], ah[1] * kw + aw[1], ah[2] * kw, aw[2])


def _splitk_floats(g):
    """Split-K scratch of a tap-grid call: the host code only splits when no tile shape gives 400 workgroups, i.e. for outputs
    below 400 * 64 px * 64 ch = 1.64 M floats, and then at most 8 ways (dam_conv.hip) -- never more than 13.1 M floats."""
    return min(8 * g.B * g.OHt * g.OWt * g.n_out, 8 * 400 * 64 * 64)


def _tapgrid(g, x, wp, y, bias=None, in_scale=None, in_shift=None, relu_in=False, res=None, res_mask=None, bn_partial=None,
             relu_out=False, batch=None, bn_bwd=None, bn_in=None):
    """dam_conv2d_tapgrid_f32 on the tap grid g -> the record count left in bn_partial."""
    parts = ctypes.c_int(0)
    ws = _workspace(y.device, _splitk_floats(g))
    st = _lib.lib().dam_conv2d_tapgrid_f32(
        _lib.ptr(x), *g[:5], _lib.ptr(wp), g.k_chunks, g.n_out, _lib.ptr(bias), _lib.ptr(in_scale), _lib.ptr(in_shift),
        1 if relu_in else 0, 1 if relu_out else 0, _lib.ptr(y), *g[7:], _lib.ptr(res), _lib.ptr(res_mask), _lib.ptr(bn_partial),
        ctypes.byref(parts) if bn_partial is not None else None, ctypes.byref(bn_bwd) if bn_bwd is not None else None,
        ctypes.byref(bn_in) if bn_in is not None else None, _lib.ptr(ws), ws.numel(), ctypes.addressof(batch) if batch is not None else None, _lib.stream())
    _lib.check(st, 'dam_conv2d_tapgrid_f32')
    return parts.value


def _tapgrid_plan(g, relu_in=False, relu_out=False, **given):
    """dam_conv2d_tapgrid_plan on the tap grid g with the operands named in `given` (keys of _HAS) -> (ConvLaunch, record count):
    what _tapgrid with those operands would launch and report.  Host arithmetic in the library; no tensor, no GPU."""
    has = _HAS['workspace']
    for name, v in given.items():
        has |= _HAS[name] if _given(v) else 0
    rec, parts = (ctypes.c_int * 16)(), ctypes.c_int(0)
    st = _lib.lib().dam_conv2d_tapgrid_plan(*g[:7], 1 if relu_in else 0, 1 if relu_out else 0, *g[7:], has, _splitk_floats(g),
                                            rec, ctypes.byref(parts))
    _lib.check(st, 'dam_conv2d_tapgrid_plan')
    return ConvLaunch(CONV_FAMILIES[rec[0]], *rec[1:14]), parts.value


def conv2d_fwd(x, wp, n_out, kh, kw, stride=1, pad=0, dil=1, bias=None, in_scale=None, in_shift=None,
               relu_in=False, in_nchw=False, bn_partial=None, bn=None, res=None, relu_out=False, finalize=True, out=None):
    """x: NHWC [B,H,W,C] (C % 16 == 0), or NCHW [B,C,H,W] with C <= 16 if in_nchw.  Returns NHWC
    [B,Ho,Wo,n_out] with n_out rounded up to a multiple of 16 (extra channels are zero).
    res (same shape as the result) is added, relu_out applies max(., 0) last: with an eval-mode BatchNorm folded into
    the weights and `bias`, one launch is relu(bn(conv(x)) [+ shortcut]).
    out: the result tensor to write (contiguous float32 [B,Ho,Wo,n16] on x's device) instead of a fresh one."""
    _lib.require_cuda(x, wp)
    _f32c(x, 'x'), _f32c(bias, 'bias'), _f32c(in_scale, 'in_scale'), _f32c(in_shift, 'in_shift'), _f32c(res, 'res')
    g = _fwd_grid(x.shape, n_out, kh, kw, stride, pad, dil, in_nchw)
    B, Ho, Wo, n16 = g.B, g.Ho, g.Wo, g.n_out
    if out is None:
        y = torch.empty((B, Ho, Wo, n16), dtype=torch.float32, device=x.device)
    else:
        if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (B, Ho, Wo, n16) or out.device != x.device:
            raise ValueError('out must be a contiguous float32 tensor of shape %s on %s' % ((B, Ho, Wo, n16), x.device))
        y = out
    parts = _tapgrid(g, x, wp, y, bias, in_scale, in_shift, relu_in, res=res, bn_partial=bn_partial, relu_out=relu_out)
    if bn is not None and bn_partial is not None:
        # two-launch form: merge the records with the finalize kernel
        out4 = bn_finalize(bn_partial, parts, *bn) if parts > 0 and finalize else None
        return y, parts, out4    # parts == 0: no statistics from this launch (out4 is then unset); finalize=False: the caller
        #                          hands (bn_partial, parts) to bn_finalize_apply
    if bn_partial is not None:
        return y, parts          # parts == 0: the launch could not produce the statistics
    return y


CONV_FAMILIES = ('none', 'strip', 'pipe', 'pipe_ranges', 'tile', 'tile_batch', '1x1')
ConvLaunch = collections.namedtuple('ConvLaunch', 'family MB NB NCH T33 LW EPI SO PU STATS KS ksplit ranges BNF')


def conv_last_launch():
    """Which kernel the last tap-grid convolution call of this thread launched (dam_conv_last_launch): the family by name and
    the template parameters of the instantiation; fields that do not belong to the family are 0.  Host-side only."""
    v = (ctypes.c_int * 16)()
    _lib.check(_lib.lib().dam_conv_last_launch(v), 'dam_conv_last_launch')
    return ConvLaunch(CONV_FAMILIES[v[0]], *v[1:14])


def conv2d_fwd_plan(x_shape, n_out, kh, kw, stride=1, pad=0, dil=1, bias=None, in_scale=None, in_shift=None, relu_in=False,
                    in_nchw=False, bn_partial=None, res=None, relu_out=False, parts=False):
    """What conv2d_fwd would launch for an input of x_shape, as conv_last_launch() would report it after the call -- decided by
    host arithmetic in the library (dam_conv2d_tapgrid_plan): no tensors, no GPU.  The keywords mean what they mean to
    conv2d_fwd; an optional operand is given as True (or as the tensor) / None.  parts=True: -> (ConvLaunch, record count the call
    would return for bn_partial)."""
    rec, n = _tapgrid_plan(_fwd_grid(tuple(x_shape), n_out, kh, kw, stride, pad, dil, in_nchw), relu_in, relu_out, bias=bias,
                           in_scale=in_scale, in_shift=in_shift, res=res, bn_partial=bn_partial)
    return (rec, n) if parts else rec


def _dgrad_operands(res, res_mask, bn_bwd, res_mask_bits, bn_in=None):
    """Which optional operands a stride-1 conv2d_dgrad hands to the tap-grid call (keys of _HAS)."""
    given = dict(res=res, res_mask=res_mask)
    if bn_in is not None:
        given.update(bn_in=True, bn_in_bits=bn_in[3])
    if bn_bwd is not None:
        given.update(bn_partial=True, bn_bwd=True, bwd_mask_scale=bn_bwd[3], bwd_mask_bits=bn_bwd[5] if len(bn_bwd) > 5 else None,
                     bwd_res_mask_bits=res_mask_bits)
    return given


def conv2d_dgrad_plan(dy_shape, n_in, H, W, kh, kw, stride=1, pad=0, dil=1, res=None, res_mask=None, accumulate_into=None,
                      bn_bwd=None, res_mask_bits=None, parts=False, bn_in=None):
    """What a stride-1 conv2d_dgrad would launch for a gradient of dy_shape, as conv_last_launch() would report it (see
    conv2d_fwd_plan).  bn_bwd, bn_in: the tuples conv2d_dgrad takes, their entries True (or tensors) / None; with bn_in the
    record's BNF says whether a kernel applies that BatchNorm's backward in its loaders (0: conv2d_dgrad(bn_in=) would raise).
    parts=True: -> (ConvLaunch, record count of the sums; 0 = conv2d_dgrad returns no partials)."""
    if stride != 1:
        raise ValueError('conv2d_dgrad_plan: stride-1 data gradients only')
    if _given(accumulate_into):
        res, res_mask = True, None
    rec, n = _tapgrid_plan(_dgrad_grid(tuple(dy_shape), n_in, H, W, kh, kw, 1, pad, dil),
                           **_dgrad_operands(res, res_mask, bn_bwd, res_mask_bits, bn_in))
    return (rec, n) if parts else rec


def _dgrad_axis(parity, pad, dil, k, stride):
    """Taps of one output-parity class of a strided data gradient along one axis:
    returns (count, k0, kstep, in_off, in_step) or None if the class receives nothing."""
    valid = [t for t in range(k) if (parity + pad - t * dil) % stride == 0]
    if not valid:
        return None
    k0 = valid[0]
    kstep = valid[1] - valid[0] if len(valid) > 1 else 1
    return len(valid), k0, kstep, (parity + pad - k0 * dil) // stride, -(kstep * dil) // stride


def conv2d_dgrad(dy, wpt, n_in, H, W, kh, kw, stride=1, pad=0, dil=1, res=None, res_mask=None, accumulate_into=None,
                 bn_bwd=None, res_mask_bits=None, pair_1x1=None, _s2_sums=None, out=None, records=None, bn_in=None):
    """dy: NHWC [B,Ho,Wo,Cout]; wpt packed with transpose=True.  Returns dx NHWC [B,H,W,n_in16]
    (+ res * (res_mask > 0) if given).  With accumulate_into=dx0 the result is added to dx0 in place.
    bn_bwd=(x, save_mean, save_invstd, mask_scale, mask_shift[, mask_bits]) (stride 1; 3x3 / stride 2 / pad 1 with the mask_bits
    form): dx is the gradient reaching relu(bn(x)) (or, with
    mask_bits and scale = shift = None, relu(bn(x) + shortcut) whose sign bytes they are); returns
    (dx, partials) where partials = (records, count) for bn_backward(partials=) when the launch could also take that
    BatchNorm's two backward sums from its epilogue, else None (stride 1; with a residual only when its mask is also given
    as the sign bytes of bn_apply, res_mask_bits -- the float res_mask serves the launches that cannot use them).
    bn_in=(c, coef, mask_affine, mask_bits) (with bn_bwd at stride 1, where conv2d_dgrad_plan reports BNF): dy is the gradient
    reaching relu(bn(c)) [+ shortcut] with the mask as mask_affine=(scale, shift) or as sign bytes, coef from
    bn_backward_finalize; the launch applies that BatchNorm's backward in its loaders and returns (dx, partials, dc), dc being
    what bn_backward would have returned as dx.
    out: the result tensor to write (contiguous float32 [B,H,W,n_in16] on dy's device) instead of a fresh one.
    records (the strided bn_bwd form only): the record buffer to write (contiguous float32, at least
    dam_bn_workspace_floats(n_in16) elements, on dy's device) instead of a fresh one."""
    _lib.require_cuda(dy, wpt)
    if records is not None:
        need = _lib.lib().dam_bn_workspace_floats((n_in + 15) // 16 * 16)
        if bn_bwd is None or stride != 2:
            raise ValueError('records: only with bn_bwd at stride 2')
        if records.dtype != torch.float32 or not records.is_contiguous() or records.numel() < need or records.device != dy.device:
            raise ValueError('records must be a contiguous float32 tensor of at least %d elements on %s' % (need, dy.device))
    if out is not None:
        want = (dy.shape[0], H, W, (n_in + 15) // 16 * 16)
        if accumulate_into is not None:
            raise ValueError('out and accumulate_into exclude each other')
        if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != want or out.device != dy.device:
            raise ValueError('out must be a contiguous float32 tensor of shape %s on %s' % (want, dy.device))
    if bn_in is not None and (bn_bwd is None or stride != 1):
        raise ValueError('bn_in: with bn_bwd at stride 1 only')
    if bn_bwd is not None and stride == 2:
        # the strided form: the upstream BatchNorm is a residual block's bn2 (mask = the sign bytes of the block output); only the
        # one-launch kernels of the thin stages take its sums, (dx, None) otherwise
        if accumulate_into is not None or res is not None or len(bn_bwd) < 6 or bn_bwd[5] is None or bn_bwd[3] is not None:
            raise ValueError('bn_bwd at stride 2: mask as sign bytes, no residual / accumulation')
        xb, mean, invstd, up_bits = bn_bwd[0], bn_bwd[1], bn_bwd[2], bn_bwd[5]
        _lib.require_cuda(xb)
        n16 = (n_in + 15) // 16 * 16
        if tuple(xb.shape) != (dy.shape[0], H, W, n16):
            raise ValueError('bn_bwd: x has the shape of the data gradient')
        rec = records if records is not None else torch.empty(_lib.lib().dam_bn_workspace_floats(n16), dtype=torch.float32, device=dy.device)
        epi = _lib.BnBwdSums(_lib.ptr(xb), _lib.ptr(mean), _lib.ptr(invstd), None, None, None, _lib.ptr(up_bits))
        got = conv2d_dgrad(dy, wpt, n_in, H, W, kh, kw, stride, pad, dil, pair_1x1=pair_1x1, _s2_sums=(epi, rec), out=out)
        return got if isinstance(got, tuple) else (got, None)
    if bn_bwd is not None:
        if stride != 1 or accumulate_into is not None:
            raise ValueError('bn_bwd: stride-1 data gradients only')
        if res is not None and (res_mask is None or res_mask_bits is None):
            raise ValueError('bn_bwd with a residual: res_mask and res_mask_bits')
        _f32c(dy, 'dy'), _f32c(res, 'res'), _f32c(res_mask, 'res_mask')
        xb, mean, invstd, msc, msh = bn_bwd[:5]
        up_bits = bn_bwd[5] if len(bn_bwd) > 5 else None     # the BatchNorm's own mask as sign bytes (msc = msh = None then)
        if (up_bits is None) == (msc is None) or (up_bits is not None and res is None):
            raise ValueError('bn_bwd: the mask as (scale, shift) or -- with a residual -- as sign bytes')
        _lib.require_cuda(xb)
        B, Ho, Wo, Co = dy.shape
        n16 = (n_in + 15) // 16 * 16
        if tuple(xb.shape) != (B, H, W, n16):
            raise ValueError('bn_bwd: x has the shape of the data gradient')
        dx = out if out is not None else torch.empty((B, H, W, n16), dtype=torch.float32, device=dy.device)
        rec = torch.empty(_lib.lib().dam_bn_workspace_floats(n16), dtype=torch.float32, device=dy.device)
        epi = _lib.BnBwdSums(_lib.ptr(xb), _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(msc), _lib.ptr(msh), _lib.ptr(res_mask_bits),
                             _lib.ptr(up_bits))
        fin = dc = None
        if bn_in is not None:
            c, coef, aff, bits = bn_in
            _lib.require_cuda(c, coef)
            _f32c(c, 'c'), _f32c(coef, 'coef')
            if c.shape != dy.shape or (aff is None) == (bits is None):
                raise ValueError('bn_in: c has the shape of dy; the mask as (scale, shift) or as sign bytes')
            dc = torch.empty_like(c)
            fin = _lib.BnBwdIn(_lib.ptr(c), _lib.ptr(coef), _lib.ptr(aff[0]) if aff else None, _lib.ptr(aff[1]) if aff else None,
                               _lib.ptr(bits), _lib.ptr(dc))
        parts = _tapgrid(_dgrad_grid(dy.shape, n_in, H, W, kh, kw, 1, pad, dil), dy, wpt, dx, res=res, res_mask=res_mask,
                         bn_partial=rec, bn_bwd=epi, bn_in=fin)
        if bn_in is not None:
            return dx, ((rec, parts) if parts > 0 else None), dc
        return dx, ((rec, parts) if parts > 0 else None)
    _f32c(dy, 'dy'), _f32c(res, 'res'), _f32c(res_mask, 'res_mask')
    B, Ho, Wo, Co = dy.shape
    n16 = (n_in + 15) // 16 * 16
    if accumulate_into is not None:
        dx, res, res_mask = accumulate_into, accumulate_into, None
    else:
        dx = out if out is not None else torch.empty((B, H, W, n16), dtype=torch.float32, device=dy.device)
    if stride == 1:
        _tapgrid(_dgrad_grid(dy.shape, n_in, H, W, kh, kw, 1, pad, dil), dy, wpt, dx, res=res, res_mask=res_mask)
        return dx
    # pair_1x1=(dy2, wpt2): a SECOND operator's data gradient into the same dx -- a 1x1 / stride-`stride` / pad-0 convolution of the
    # same input (a down-sampling block's shortcut beside its conv1): its one tap lands on the pixels of this operator's single-tap
    # parity class (0, 0) and rides in that class's launch (dam_conv1x1_pair_f32) instead of a launch of its own that re-reads dx
    if pair_1x1 is not None:
        dy2, wpt2 = pair_1x1
        _lib.require_cuda(dy2, wpt2)
        _f32c(dy2, 'pair dy')
        if accumulate_into is not None or res is not None or tuple(dy2.shape) != tuple(dy.shape):
            raise ValueError('pair_1x1: a second gradient of the same shape, no residual / accumulation')
        a0 = _dgrad_axis(0, pad, dil, kh, stride), _dgrad_axis(0, pad, dil, kw, stride)
        if a0[0] is None or a0[1] is None or a0[0][0] != 1 or a0[1][0] != 1 or a0[0][3] != 0 or a0[1][3] != 0:
            raise ValueError('pair_1x1: class (0, 0) of this operator is not a single tap at offset 0')
    # 3x3 / stride 2 / pad 1 (the first convolution of a down-sampling block): all four parity classes (+ the pair term) from
    # one read of dy in one launch (dam_dgrad_s2_3x3_f32: weights resident in LDS for the thin layers, streamed from L2 for the wide)
    if (DGRAD_S2 and stride == 2 and kh == 3 and kw == 3 and pad == 1 and dil == 1 and accumulate_into is None and res is None
            and Ho == (H + 1) // 2 and Wo == (W + 1) // 2):
        parts = ctypes.c_int(0)
        st = _lib.lib().dam_dgrad_s2_3x3_f32(_lib.ptr(dy), _lib.ptr(wpt), _lib.ptr(pair_1x1[0]) if pair_1x1 else None,
                                             _lib.ptr(pair_1x1[1]) if pair_1x1 else None, B, Ho, Wo, Co, n16, _lib.ptr(dx), H, W,
                                             ctypes.byref(_s2_sums[0]) if _s2_sums else None,
                                             _lib.ptr(_s2_sums[1]) if _s2_sums else None, ctypes.byref(parts) if _s2_sums else None,
                                             _lib.stream())
        if st == 0:
            global dgrad_s2_launches
            dgrad_s2_launches += 1
            if _s2_sums:
                return dx, ((_s2_sums[1], parts.value) if parts.value > 0 else None)
            return dx
        if st != -2:                                   # DAM_ERR_UNSUPPORTED: not a layer that kernel takes -> the class launches
            _lib.check(st, 'dam_dgrad_s2_3x3_f32')
    classes = [(_dgrad_axis(ph, pad, dil, kh, stride), _dgrad_axis(pw, pad, dil, kw, stride))
               for ph in range(stride) for pw in range(stride)]
    if any(a is None or b is None for a, b in classes) and accumulate_into is None:
        if res is not None:
            raise ValueError('a fused residual needs every output parity class to receive taps')
        dx.zero_()          # classes without taps get no gradient (e.g. the 1x1 stride-2 shortcut)
    # the classes write disjoint pixels of dx from the same dy and weights: those that take the tile kernel are recorded
    # and run as ONE launch (class in blockIdx.z) at the flush
    batch = _conv_batch(dy.device)
    try:
        for ph in range(stride):
            for pw in range(stride):
                g = _dgrad_grid(dy.shape, n_in, H, W, kh, kw, stride, pad, dil, ph, pw)
                if g is None:
                    continue
                if pair_1x1 is not None and ph == 0 and pw == 0:
                    if g.Ho != Ho or g.Wo != Wo:
                        raise ValueError('pair_1x1: class (0, 0) does not cover the gradient\'s pixels')
                    _lib.check(_lib.lib().dam_conv1x1_pair_f32(_lib.ptr(dy), _lib.ptr(wpt), g.wt_base, _lib.ptr(pair_1x1[0]),
                                                               _lib.ptr(pair_1x1[1]), 0, B, Ho, Wo, Co, n16, _lib.ptr(dx), H, W, stride,
                                                               0, 0, _lib.stream()), 'dam_conv1x1_pair_f32')
                    continue
                _tapgrid(g, dy, wpt, dx, res=res, res_mask=res_mask, batch=batch)
        _lib.check(_lib.lib().dam_conv_batch_flush(ctypes.addressof(batch), _lib.stream()), 'dam_conv_batch_flush')
    except Exception:
        _lib.lib().dam_conv_batch_init(ctypes.addressof(batch))      # drop what a failed call left recorded
        raise
    return dx


_conv_batches = {}


def _conv_batch(device):
    """The device's launch batch for sibling tile-kernel launches (include/dam_hip.h: dam_conv_batch_*)."""
    key = (device.type, device.index)
    b = _conv_batches.get(key)
    if b is None:
        L = _lib.lib()
        b = _conv_batches[key] = ctypes.create_string_buffer(int(L.dam_conv_batch_bytes()))
        _lib.check(L.dam_conv_batch_init(ctypes.addressof(b)), 'dam_conv_batch_init')
    return b


_workspaces = {}
_retired = []          # superseded buffers are kept: a captured hipGraph may have their address baked in


def _grow(table, key, device, floats):
    ws = table.get(key)
    if ws is None or ws.numel() < floats:
        if ws is not None:
            _retired.append(ws)
        ws = torch.empty(int(floats), dtype=torch.float32, device=device)
        table[key] = ws
    return ws


def _workspace(device, floats):
    """One grow-only scratch buffer per device (split-K slabs, weight-gradient slabs, reduction scratch of
    the heads / mask-sum); all users of one buffer are ordered on one stream.  A buffer that has to grow is never freed:
    hipGraphs captured earlier keep replaying into the old one (the launches recorded there were sized for it)."""
    return _grow(_workspaces, (device.type, device.index), device, floats)


# Parameters and BatchNorm running statistics are updated IN PLACE by kernels of this library (the fused Adam launch, the
# statistics finalize), possibly inside a replayed hipGraph: torch's tensor version counters do not see that.  Whatever
# caches something derived from them (layers.FoldedConvBn) keys on this counter too; it is bumped by every training forward
# (the statistics finalize updates the running buffers), every optimizer launch and every graph replay of a step.
PARAM_EPOCH = 0


def params_changed():
    global PARAM_EPOCH
    PARAM_EPOCH += 1


# The equal weight gradients of a deep stage as one launch (include/dam_hip.h: dam_wgrad_queue_set_batching): every queue asks
# for it.  A constant, not a switch (the unbatched A/B lost); tests read it as their precondition.
WGRAD_BATCH = True
_wgrad_queues = {}      # device -> [ctypes buffer of the library's queue, calls recorded since the last flush]


def _wgrad_queue(device):
    key = (device.type, device.index)
    q = _wgrad_queues.get(key)
    if q is None:
        L = _lib.lib()
        buf = ctypes.create_string_buffer(int(L.dam_wgrad_queue_bytes()))
        _lib.check(L.dam_wgrad_queue_init(ctypes.addressof(buf)), 'dam_wgrad_queue_init')
        _lib.check(L.dam_wgrad_queue_set_batching(ctypes.addressof(buf), int(WGRAD_BATCH)), 'dam_wgrad_queue_set_batching')
        # [the library's queue, calls recorded since the last flush, tensors those calls read (kept alive until the flush: with
        #  batching a recorded call's slab kernel may not have been launched yet)]
        q = _wgrad_queues[key] = [buf, 0, []]
    return q


def wgrad_abandon(device=None):
    """Drops reductions that were recorded but never flushed -- a backward pass that raised half-way leaves them behind,
    and the next step's jobs would target the same gradients from the same flush launch.  Called at the start of every
    step (optim.Adam.zero_grad, engine.TrainStep); a no-op in the normal case."""
    for key, q in _wgrad_queues.items():
        if q[1] and (device is None or key == (device.type, device.index)):
            _lib.check(_lib.lib().dam_wgrad_queue_init(ctypes.addressof(q[0])), 'dam_wgrad_queue_init')
            del q[2][:]
            q[1] = 0


def wgrad_flush(device=None):
    """Runs the slab reductions recorded by conv2d_wgrad(..., defer=True) in one launch on the current stream; the
    gradients are in their `out` buffers when that launch is done.  No-op when nothing is recorded."""
    for key, q in _wgrad_queues.items():
        if q[1] and (device is None or key == (device.type, device.index)):
            _lib.check(_lib.lib().dam_wgrad_queue_flush(ctypes.addressof(q[0]), _lib.stream()), 'dam_wgrad_queue_flush')
            q[1] = 0
            del q[2][:]


def _wgrad_call(x_shape, dy_shape, n_out, kh, kw, in_nchw, c_real):
    """-> (B, H, W, C, Ho, Wo, n_chan, c_real or C, workspace floats) of a weight-gradient call: the shape unpacking and the
    workspace size conv2d_wgrad and conv2d_wgrad_plan share."""
    if in_nchw:
        B, C, H, W = x_shape
    else:
        B, H, W, C = x_shape
    _, Ho, Wo, n_chan = dy_shape
    floats = _lib.lib().dam_conv2d_wgrad_workspace_floats(n_out, C, kh, kw)
    return B, H, W, C, Ho, Wo, n_chan, C if c_real is None else int(c_real), floats


def conv2d_wgrad(x, dy, n_out, kh, kw, stride=1, pad=0, dil=1, in_scale=None, in_shift=None, relu_in=False,
                 in_nchw=False, out=None, c_real=None, defer=False, batch_rows=False):
    """dW in torch layout [n_out, c_real or C, kh, kw] from x (NHWC, or NCHW first layer) and dy NHWC [B,Ho,Wo,n16].
    out: where to write it (e.g. the parameter's slice of a flat gradient buffer).
    defer (needs out): only the slab kernel runs now; the reduction into `out` is recorded and happens in wgrad_flush(),
    one launch for every weight gradient of the backward pass (each deferred call keeps its own slab buffer until then).
    batch_rows (with defer): a call that takes the stride-1 row kernel is recorded as well and runs with the other recorded
    calls of its instantiation and geometry as ONE launch -- when another kind arrives, when the job table is full or at
    wgrad_flush() (dam_wgrad_queue_set_batching mode 2).  x, dy and the affine must then stay UNMODIFIED until the flush (the
    queue keeps them alive, it cannot keep them from being written in place).  Without it such a call is launched at once."""
    _lib.require_cuda(x, dy)
    _f32c(x, 'x'), _f32c(dy, 'dy')
    B, H, W, C, Ho, Wo, n_chan, cr, floats = _wgrad_call(x.shape, dy.shape, n_out, kh, kw, in_nchw, c_real)
    L = _lib.lib()
    if out is None:
        if defer:
            raise ValueError('a deferred weight gradient needs the buffer it will be written to')
        out = torch.empty((n_out, cr, kh, kw), dtype=torch.float32, device=x.device)
    elif out.numel() != n_out * cr * kh * kw or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError('bad out tensor for the weight gradient')
    if defer:
        q = _wgrad_queue(x.device)
        ws = _grow(_workspaces, (x.device.type, x.device.index, 'wgrad slabs', q[1]), x.device, floats)
        q[1] += 1
        q[2].append((x, dy, in_scale, in_shift))
        queue = ctypes.addressof(q[0])
        if WGRAD_BATCH:        # the mode is that of the NEXT call: row launches wait for each other only where the caller asked
            _lib.check(L.dam_wgrad_queue_set_batching(queue, 2 if batch_rows else 1), 'dam_wgrad_queue_set_batching')
    else:
        ws, queue = _workspace(x.device, floats), None
    _lib.check(L.dam_conv2d_wgrad_f32(_lib.ptr(x), B, H, W, C, 1 if in_nchw else 0, _lib.ptr(in_scale),
                                      _lib.ptr(in_shift), 1 if relu_in else 0, _lib.ptr(dy), Ho, Wo, n_chan, n_out,
                                      kh, kw, stride, pad, dil, _lib.ptr(out), cr, _lib.ptr(ws), ws.numel(), queue,
                                      _lib.stream()), 'dam_conv2d_wgrad_f32')
    return out


WGRAD_FAMILIES = ('none', 'rows', 'rows_s2', 'direct', 'tile')
WgradLaunch = collections.namedtuple('WgradLaunch', 'family TNB TKB STEPS KP GPP GPPD HV NL TA TB nx nsplit spi rps TMW issued')


def _wgrad_launch(v):
    """The 16 ints of dam_wgrad_last_launch / dam_conv2d_wgrad_plan as a WgradLaunch."""
    fam = WGRAD_FAMILIES[v[0]]
    rows = fam in ('rows', 'rows_s2')
    return WgradLaunch(fam, *v[1:13], v[13] if rows else 0, v[14] if rows else 0, v[13] if fam == 'tile' else 0, v[15])


def wgrad_last_launch():
    """Which kernel the last conv2d_wgrad call of this thread committed to (dam_wgrad_last_launch): the family by name, the
    template parameters of the instantiation (rows_s2: GPP is GPPX; direct: TA, TB are KH, KW), the grid (nx, nsplit), strips per
    image and rows per strip (row kernels) or pixels per tile (tile kernel), and how it was issued (0 launched and reduced now,
    1 launched with the reduction queued, 2 the launch itself recorded for a batched launch at the flush or earlier); fields that do not
    belong to the family are 0.  Host-side only."""
    v = (ctypes.c_int * 16)()
    _lib.check(_lib.lib().dam_wgrad_last_launch(v), 'dam_wgrad_last_launch')
    return _wgrad_launch(v)


def conv2d_wgrad_plan(x_shape, dy_shape, n_out, kh, kw, stride=1, pad=0, dil=1, affine=False, relu_in=False, in_nchw=False,
                      c_real=None, defer=False, workspace_floats=None, batch_rows=False):
    """The WgradLaunch wgrad_last_launch() would report after conv2d_wgrad on tensors of these shapes, with in_scale and in_shift
    given (affine) or not: host arithmetic in the library (dam_conv2d_wgrad_plan), no tensors, no GPU.  defer: the call goes to
    this package's queue (batch_rows: as in conv2d_wgrad); workspace_floats: None for the workspace conv2d_wgrad passes.  Raises where the call would be refused
    for its arguments or its workspace."""
    B, H, W, C, Ho, Wo, n_chan, cr, floats = _wgrad_call(x_shape, dy_shape, n_out, kh, kw, in_nchw, c_real)
    v = (ctypes.c_int * 16)()
    _lib.check(_lib.lib().dam_conv2d_wgrad_plan(B, H, W, C, 1 if in_nchw else 0, 1 if relu_in else 0, Ho, Wo, n_chan, n_out, kh, kw,
                                                stride, pad, dil, cr, 1 if affine else 0, 1 if affine else 0,
                                                ((4 if batch_rows else 2) if WGRAD_BATCH else 1) if defer else 0,
                                                floats if workspace_floats is None else int(workspace_floats), v),
               'dam_conv2d_wgrad_plan')
    return _wgrad_launch(v)


S2_ENTRIES = ('none', 'pair_fwd', 'dgrad_s2', 'pair_1x1')
S2_FAMILIES = ('none', 'resident', 'stream_lds', 'stream', 'pair_1x1')
S2Launch = collections.namedtuple('S2Launch', 'entry family NB NCH MB WAVES pair sums workgroups units rounds n_xcd records')


def s2_last_launch():
    """Which kernel the last conv_s2_pair_fwd / strided conv2d_dgrad call of this thread launched (dam_s2_last_launch): the entry
    point and the kernel family by name, the template parameters of the instantiation (1x1 pair: WAVES is R, pair is BOTH), the
    grid, the wave units, the largest number of units one wave takes (rounds), the XCD split and the records written; entry
    'none' after a call that was refused.  Host-side only."""
    v = (ctypes.c_int * 16)()
    _lib.check(_lib.lib().dam_s2_last_launch(v), 'dam_s2_last_launch')
    return _s2_launch(v)


def _s2_launch(v):
    return S2Launch(S2_ENTRIES[v[0]], S2_FAMILIES[v[1]], *v[2:13])


def _s2_plan(name, *scalars):
    """A plan entry of the down-sampling block's kernels -> S2Launch.  A refusal (DAM_ERR_UNSUPPORTED) is an answer -- the 'none'
    record: the caller falls back; bad arguments raise."""
    v = (ctypes.c_int * 16)()
    st = getattr(_lib.lib(), name)(*[int(s) for s in scalars], v)
    if st != -2:
        _lib.check(st, name)
    return _s2_launch(v)


def conv_s2_pair_fwd_plan(x_shape, n_out, stats=True, cus=0, resident=0):
    """The S2Launch s2_last_launch() would report after conv_s2_pair_fwd on an NHWC x of this shape ('none': the call returns None):
    host arithmetic in the library (dam_conv_s2_pair_fwd_plan), no tensors.  cus, resident: the device's CU count and the
    workgroups of the persistent kernel a CU holds; both given, no GPU is asked; 0: the current device's, as the call takes them."""
    B, H, W, C = x_shape
    return _s2_plan('dam_conv_s2_pair_fwd_plan', B, H, W, C, (n_out + 15) // 16 * 16, bool(stats), cus, resident)


def conv2d_dgrad_s2_plan(dy_shape, n_in, H, W, pair=False, sums=False, cus=0, resident=0):
    """The S2Launch the one-launch 3x3 / stride-2 / pad-1 data gradient (dam_dgrad_s2_3x3_f32, the first thing a strided
    conv2d_dgrad tries) would leave for a gradient of dy_shape, with pair_1x1 (pair) and the strided bn_bwd form (sums) given or
    not; 'none': refused, conv2d_dgrad runs the parity classes (+ conv1x1_pair_plan's launch).  cus, resident: as
    conv_s2_pair_fwd_plan."""
    B, Hd, Wd, Co = dy_shape
    return _s2_plan('dam_dgrad_s2_3x3_plan', B, Hd, Wd, Co, (n_in + 15) // 16 * 16, H, W, bool(pair), bool(sums), cus, resident)


def conv1x1_pair_plan(dy_shape, n_in, H, W, stride=2, off_h=0, off_w=0):
    """The S2Launch of the 1x1 pair launch (dam_conv1x1_pair_f32) that carries parity class (0, 0) of a strided conv2d_dgrad with
    pair_1x1: two single-tap operators on gradients of dy_shape into the pixels (off + stride * i) of a [B, H, W, n_in16] dx."""
    B, Ho, Wo, Co = dy_shape
    return _s2_plan('dam_conv1x1_pair_plan', B, Ho, Wo, Co, (n_in + 15) // 16 * 16, H, W, stride, off_h, off_w)


def nchw_to_nhwc16(x):
    """[B,C,H,W] float32 (C <= 16) -> NHWC [B,H,W,16], channels C..15 zero."""
    _lib.require_cuda(x)
    _f32c(x, 'x')
    B, C, H, W = x.shape
    y = torch.empty((B, H, W, 16), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dam_nchw_to_nhwc16_f32(_lib.ptr(x), B, C, H * W, _lib.ptr(y), _lib.stream()), 'dam_nchw_to_nhwc16_f32')
    return y


# ----------------------------------------------------------------------------- batch norm
def _bn_ws(device, C):
    return _workspace(device, _lib.lib().dam_bn_workspace_floats(C))


_bn_partials = {}


def bn_stats(x, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps):
    """Training-mode statistics of NHWC x.  Returns (save_mean, save_invstd, scale, shift), updates the running buffers."""
    _lib.require_cuda(x)
    C = x.shape[-1]
    P = x.numel() // C
    out = torch.empty((4, C), dtype=torch.float32, device=x.device)
    ws = _bn_ws(x.device, C)
    _lib.check(_lib.lib().dam_bn_stats_f32(_lib.ptr(x), P, C, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(running_mean),
                                           _lib.ptr(running_var), _lib.ptr(num_batches_tracked), float(momentum), float(eps),
                                           _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.ptr(out[3]),
                                           _lib.ptr(ws), _lib.stream()), 'dam_bn_stats_f32')
    return out[0], out[1], out[2], out[3]


def bn_stats_partial(x):
    """The partial statistics records of NHWC x alone: (records, count) for bn_finalize_apply / bn_finalize."""
    _lib.require_cuda(x)
    C = x.shape[-1]
    ws = bn_partial_buffer(x.device, C)
    parts = ctypes.c_int(0)
    _lib.check(_lib.lib().dam_bn_stats_partial_f32(_lib.ptr(x), x.numel() // C, C, _lib.ptr(ws), ctypes.byref(parts), _lib.stream()),
               'dam_bn_stats_partial_f32')
    return ws, parts.value


def bn_finalize_apply(partial, parts, bn, x, relu=True, res=None, res_scale=None, res_shift=None, sign_bits=False):
    """bn_finalize + bn_apply in ONE launch (dam_bn_finalize_apply_f32): bn = (gamma, beta, running_mean, running_var,
    num_batches_tracked, momentum, eps).  Returns ((save_mean, save_invstd, scale, shift), y or (y, bits))."""
    _lib.require_cuda(partial, x)
    C = x.shape[-1]
    out4 = torch.empty((4, C), dtype=torch.float32, device=x.device)
    fin = _bn_fin_struct(bn, out4)
    y = torch.empty_like(x)
    bits = torch.empty(x.shape[:-1] + (C // 4,), dtype=torch.uint8, device=x.device) if sign_bits else None
    _lib.check(_lib.lib().dam_bn_finalize_apply_f32(_lib.ptr(partial), int(parts), C, ctypes.byref(fin), _lib.ptr(x), x.numel() // C,
                                                    _lib.ptr(res), _lib.ptr(res_scale), _lib.ptr(res_shift), 1 if relu else 0,
                                                    _lib.ptr(y), _lib.ptr(bits), _lib.stream()), 'dam_bn_finalize_apply_f32')
    return (out4[0], out4[1], out4[2], out4[3]), ((y, bits) if sign_bits else y)


def bn_partial_buffer(device, C):
    """The BatchNorm partial records a convolution launch can emit: a buffer of their own per device and width (they
    live from the convolution launch to the finalize launch and must not alias any kernel's scratch)."""
    return _grow(_bn_partials, (device.type, device.index, C), device, _lib.lib().dam_bn_workspace_floats(C))


def bn_stats_pair(xa, bn_a, xb, bn_b):
    """bn_stats for two tensors of one shape in one partial + one finalize launch.  bn_a, bn_b = (gamma, beta, running_mean,
    running_var, num_batches_tracked, momentum, eps).  Returns two (save_mean, save_invstd, scale, shift) tuples."""
    _lib.require_cuda(xa, xb)
    if xa.shape != xb.shape:
        raise ValueError('the two tensors of a pair have the same shape')
    C = xa.shape[-1]
    L = _lib.lib()
    outs = [torch.empty((4, C), dtype=torch.float32, device=xa.device) for _ in range(2)]
    fa, fb = _bn_fin_struct(bn_a, outs[0]), _bn_fin_struct(bn_b, outs[1])
    ws = _workspace(xa.device, 2 * L.dam_bn_workspace_floats(C))
    _lib.check(L.dam_bn_stats_pair_f32(_lib.ptr(xa), _lib.ptr(xb), xa.numel() // C, C, ctypes.byref(fa), ctypes.byref(fb),
                                       _lib.ptr(ws), _lib.stream()), 'dam_bn_stats_pair_f32')
    return tuple(outs[0]), tuple(outs[1])


def conv_s2_pair_fwd(x, wp, wp_sc, n_out, stats=True, out=None, records=None):
    """conv1 (3x3 / stride 2 / pad 1) and the 1x1 / stride-2 shortcut convolution of one NHWC input in one launch:
    (c1, cs, (records1, records_sc, parts) or None), or None when the layer is not one dam_conv_s2_pair_fwd_f32 takes.
    out=(c1, cs): the result tensors to write (contiguous float32 [B,Hd,Wd,n_out16] on x's device) instead of fresh ones;
    records=(p1, p2) (with stats): the record buffers to write (contiguous float32, at least dam_bn_workspace_floats(n_out16)
    elements each, on x's device) instead of fresh ones."""
    _lib.require_cuda(x, wp, wp_sc)
    _f32c(x, 'x')
    B, H, W, C = x.shape
    n16 = (n_out + 15) // 16 * 16
    Hd, Wd = (H + 1) // 2, (W + 1) // 2
    if out is not None:
        want = (B, Hd, Wd, n16)
        if len(out) != 2 or any(t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != want or t.device != x.device
                                for t in out):
            raise ValueError('out must be two contiguous float32 tensors of shape %s on %s' % (want, x.device))
        c1, cs = out
    else:
        c1 = torch.empty((B, Hd, Wd, n16), dtype=torch.float32, device=x.device)
        cs = torch.empty_like(c1)
    p1 = p2 = None
    parts = ctypes.c_int(0)
    if records is not None and not stats:
        raise ValueError('records: only with stats')
    if stats:
        n = _lib.lib().dam_bn_workspace_floats(n16)
        if records is not None:
            if len(records) != 2 or any(t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n or t.device != x.device
                                        for t in records):
                raise ValueError('records must be two contiguous float32 tensors of at least %d elements on %s' % (n, x.device))
            p1, p2 = records
        else:
            p1 = torch.empty(n, dtype=torch.float32, device=x.device)
            p2 = torch.empty(n, dtype=torch.float32, device=x.device)
    st = _lib.lib().dam_conv_s2_pair_fwd_f32(_lib.ptr(x), _lib.ptr(wp), _lib.ptr(wp_sc), B, H, W, C, n16, _lib.ptr(c1), _lib.ptr(cs),
                                             _lib.ptr(p1), _lib.ptr(p2), ctypes.byref(parts), _lib.stream())
    if st == -2:                                       # DAM_ERR_UNSUPPORTED
        return None
    _lib.check(st, 'dam_conv_s2_pair_fwd_f32')
    return c1, cs, ((p1, p2, parts.value) if stats else None)


def bn_finalize_pair(partial_a, partial_b, parts, bn_a, bn_b):
    """bn_finalize for two BatchNorms whose records have one count (conv_s2_pair_fwd): one launch.  bn_a, bn_b as bn_stats_pair.
    Returns two (save_mean, save_invstd, scale, shift) tuples."""
    C = bn_a[0].numel()
    outs = [torch.empty((4, C), dtype=torch.float32, device=partial_a.device) for _ in range(2)]
    fa, fb = _bn_fin_struct(bn_a, outs[0]), _bn_fin_struct(bn_b, outs[1])
    _lib.check(_lib.lib().dam_bn_finalize_pair_f32(_lib.ptr(partial_a), _lib.ptr(partial_b), parts, C, ctypes.byref(fa),
                                                   ctypes.byref(fb), _lib.stream()), 'dam_bn_finalize_pair_f32')
    return tuple(outs[0]), tuple(outs[1])


def bn_finalize(partial, parts, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps):
    """Merges `parts` partial records (from conv2d_fwd(..., bn_partial=...)) -> (save_mean, save_invstd, scale, shift)."""
    C = gamma.numel()
    out = torch.empty((4, C), dtype=torch.float32, device=gamma.device)
    _lib.check(_lib.lib().dam_bn_finalize_f32(_lib.ptr(partial), parts, C, _lib.ptr(gamma), _lib.ptr(beta),
                                              _lib.ptr(running_mean), _lib.ptr(running_var), _lib.ptr(num_batches_tracked),
                                              float(momentum), float(eps), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]),
                                              _lib.ptr(out[3]), _lib.stream()), 'dam_bn_finalize_f32')
    return out[0], out[1], out[2], out[3]


def bn_eval_affine(gamma, beta, running_mean, running_var, eps):
    _lib.require_cuda(gamma)
    C = gamma.numel()
    out = torch.empty((4, C), dtype=torch.float32, device=gamma.device)
    _lib.check(_lib.lib().dam_bn_eval_affine_f32(C, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(running_mean),
                                                 _lib.ptr(running_var), float(eps), _lib.ptr(out[0]), _lib.ptr(out[1]),
                                                 _lib.ptr(out[2]), _lib.ptr(out[3]), _lib.stream()), 'dam_bn_eval_affine_f32')
    return out[0], out[1], out[2], out[3]


def bn_apply(x, scale, shift, relu=True, res=None, res_scale=None, res_shift=None, sign_bits=False):
    """y = relu?(x*scale + shift [+ res [*res_scale + res_shift]]).  sign_bits=True: returns (y, bits) with one uint8 per
    channel quad, bit i = (y[..., 4q + i] > 0): what bn_backward(mask_bits=) reads instead of y."""
    _lib.require_cuda(x)
    C = x.shape[-1]
    y = torch.empty_like(x)
    bits = torch.empty(x.shape[:-1] + (C // 4,), dtype=torch.uint8, device=x.device) if sign_bits else None
    _lib.check(_lib.lib().dam_bn_apply_f32(_lib.ptr(x), x.numel() // C, C, _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(res),
                                           _lib.ptr(res_scale), _lib.ptr(res_shift), 1 if relu else 0, _lib.ptr(y),
                                           _lib.ptr(bits), _lib.stream()), 'dam_bn_apply_f32')
    return (y, bits) if sign_bits else y


def bn_backward_pair(dy, y_mask, a, b, training=True, mask_bits=None):
    """bn_backward for two BatchNorms fed by the same dy through the same ReLU mask (a residual block's bn2 and its shortcut
    BatchNorm): three launches instead of six, dy / y_mask read once per pass.  a, b = (x, gamma, save_mean, save_invstd,
    dgamma or None, dbeta or None).  Returns ((dx, dgamma, dbeta), (dx, dgamma, dbeta)), bitwise equal to two bn_backward calls."""
    _lib.require_cuda(dy, a[0], b[0])
    if (y_mask is None) == (mask_bits is None):
        raise ValueError('exactly one of y_mask / mask_bits')
    C = a[0].shape[-1]
    if b[0].shape != a[0].shape or dy.shape != a[0].shape:
        raise ValueError('the two BatchNorms of a pair see the same shape')
    outs = []
    for x, gamma, mean, invstd, dgamma, dbeta in (a, b):
        dx = torch.empty_like(x)
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device) if dgamma is None else dgamma
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device) if dbeta is None else dbeta
        outs.append((dx, dgamma, dbeta))
    L = _lib.lib()
    ws = _workspace(dy.device, L.dam_bn_pair_workspace_floats(C))
    args = []
    for (x, gamma, mean, invstd, _, _), (dx, dgamma, dbeta) in zip((a, b), outs):
        args += [_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta)]
    _lib.check(L.dam_bn_backward_pair_f32(_lib.ptr(dy), _lib.ptr(y_mask), _lib.ptr(mask_bits), dy.numel() // C, C,
                                          1 if training else 0, *args,
                                          _lib.ptr(ws), _lib.stream()), 'dam_bn_backward_pair_f32')
    return outs[0], outs[1]


def bn_backward(dy, y_mask, x, gamma, save_mean, save_invstd, training=True, mask_affine=None, dgamma=None, dbeta=None,
                mask_bits=None, partials=None):
    """Returns (dx, dgamma, dbeta) for y = [relu](bn(x) + ...).  The ReLU mask comes from y_mask (the saved output), or --
    for a plain relu(bn(x)) -- from mask_affine=(scale, shift), the forward's fused affine (the saved output is not read),
    or there is none (both None)."""
    _lib.require_cuda(dy, x)
    C = x.shape[-1]
    dx = torch.empty_like(x)
    # two separate allocations: autograd takes ownership of a whole tensor it is handed as a .grad, but clones a view
    # (30 extra device copies per ResNet18 step when these were rows of one [2, C] tensor)
    if dgamma is None:
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
    if dbeta is None:
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
    # partials=(records, count) from conv2d_dgrad(bn_bwd=): the two sums are already there, only finalize + apply run
    ws, given = (_bn_ws(x.device, C), 0) if partials is None else partials
    _lib.check(_lib.lib().dam_bn_backward_f32(_lib.ptr(dy), _lib.ptr(y_mask), _lib.ptr(x), x.numel() // C, C, _lib.ptr(gamma),
                                              _lib.ptr(save_mean), _lib.ptr(save_invstd), 1 if training else 0,
                                              _lib.ptr(mask_affine[0]) if mask_affine else None,
                                              _lib.ptr(mask_affine[1]) if mask_affine else None, _lib.ptr(mask_bits), _lib.ptr(dx),
                                              _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(ws), given, _lib.stream()),
               'dam_bn_backward_f32')
    return dx, dgamma, dbeta


def bn_backward_finalize(partials, x, gamma, save_mean, save_invstd, training=True, dgamma=None, dbeta=None):
    """The finalize of bn_backward(partials=) on its own: -> (coef [3, C], dgamma, dbeta), dgamma / dbeta bitwise bn_backward's;
    coef is what conv2d_dgrad(bn_in=) applies in its loaders (x: the BatchNorm's input, for its shape only)."""
    _lib.require_cuda(x, gamma)
    C = x.shape[-1]
    if dgamma is None:
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
    if dbeta is None:
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
    coef = torch.empty((3, C), dtype=torch.float32, device=x.device)
    ws, given = partials
    _lib.check(_lib.lib().dam_bn_backward_finalize_f32(_lib.ptr(ws), given, x.numel() // C, C, _lib.ptr(gamma), _lib.ptr(save_mean),
                                                       _lib.ptr(save_invstd), 1 if training else 0, _lib.ptr(dgamma),
                                                       _lib.ptr(dbeta), _lib.ptr(coef), _lib.stream()),
               'dam_bn_backward_finalize_f32')
    return coef, dgamma, dbeta


def channel_sum(x, n_real, out=None):
    _lib.require_cuda(x)
    C = x.shape[-1]
    if out is None:
        out = torch.empty(n_real, dtype=torch.float32, device=x.device)
    ws = _bn_ws(x.device, C)
    _lib.check(_lib.lib().dam_channel_sum_f32(_lib.ptr(x), x.numel() // C, C, n_real, _lib.ptr(out), _lib.ptr(ws),
                                              _lib.stream()), 'dam_channel_sum_f32')
    return out


# ----------------------------------------------------------------------------- heads / mask-sum / loss
def heads_fwd(trunk, conv_w, conv_b, fc_w, fc_b):
    """trunk NHWC [B,h,w,C]; conv_w [S,C]; conv_b [S]; fc_w [S,P]; fc_b [S] -> (h [B,S,P], gains [B,S])."""
    _lib.require_cuda(trunk)
    B, C = trunk.shape[0], trunk.shape[-1]
    P = trunk.numel() // (B * C)
    S = conv_w.shape[0]
    if fc_w.shape != (S, P):
        raise ValueError('fc_head expects %d inputs but the trunk gives %d (flattened_dim mismatch)' % (fc_w.shape[1], P))
    h = torch.empty((B, S, P), dtype=torch.float32, device=trunk.device)
    g = torch.empty((B, S), dtype=torch.float32, device=trunk.device)
    _lib.check(_lib.lib().dam_heads_fwd_f32(_lib.ptr(trunk), B, P, C, S, _lib.ptr(conv_w), _lib.ptr(conv_b), _lib.ptr(fc_w),
                                            _lib.ptr(fc_b), _lib.ptr(h), _lib.ptr(g), _lib.stream()), 'dam_heads_fwd_f32')
    return h, g


def heads_bwd(dgains, h, trunk, conv_w, fc_w, outs=None):
    """outs: optional (dconv_w [S,C], dconv_b [S], dfc_w [S,P], dfc_b [S]) destinations (gradient slots)."""
    B, S, P = h.shape
    C = trunk.shape[-1]
    dev = trunk.device
    dtrunk = torch.empty_like(trunk)
    o = outs or (None, None, None, None)
    dcw = o[0] if o[0] is not None else torch.empty((S, C), dtype=torch.float32, device=dev)
    dcb = o[1] if o[1] is not None else torch.empty(S, dtype=torch.float32, device=dev)
    dfw = o[2] if o[2] is not None else torch.empty((S, P), dtype=torch.float32, device=dev)
    dfb = o[3] if o[3] is not None else torch.empty(S, dtype=torch.float32, device=dev)
    L = _lib.lib()
    ws = _workspace(dev, L.dam_heads_bwd_workspace_floats(B, P, C, S))
    _lib.check(L.dam_heads_bwd_f32(_lib.ptr(dgains), _lib.ptr(h), _lib.ptr(trunk), B, P, C, S, _lib.ptr(conv_w), _lib.ptr(fc_w),
                                   _lib.ptr(dtrunk), _lib.ptr(dcw), _lib.ptr(dcb), _lib.ptr(dfw), _lib.ptr(dfb), _lib.ptr(ws),
                                   _lib.stream()), 'dam_heads_bwd_f32')
    return dtrunk, dcw, dcb, dfw, dfb


def masksum_fwd(x, gains):
    """x [B,S,F,T], gains [B,S] -> masked [B,F,T]."""
    _lib.require_cuda(x, gains)
    B, S, F, T = x.shape
    masked = torch.empty((B, F, T), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dam_masksum_fwd_f32(_lib.ptr(x), _lib.ptr(gains), B, S, F * T, _lib.ptr(masked), _lib.stream()),
               'dam_masksum_fwd_f32')
    return masked


def masksum_bwd(dmasked, x):
    B, S, F, T = x.shape
    dg = torch.empty((B, S), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    ws = _workspace(x.device, L.dam_masksum_workspace_floats(B, S))
    _lib.check(L.dam_masksum_bwd_f32(_lib.ptr(dmasked), _lib.ptr(x), B, S, F * T, _lib.ptr(dg), _lib.ptr(ws), _lib.stream()),
               'dam_masksum_bwd_f32')
    return dg


def masksum_mse(x, gains, gt, want_masked=True):
    """Fused masked-sum + MSE: returns (masked or None, loss [1], dloss/dgains [B,S])."""
    _lib.require_cuda(x, gains, gt)
    B, S, F, T = x.shape
    dev = x.device
    masked = torch.empty((B, F, T), dtype=torch.float32, device=dev) if want_masked else None
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dg = torch.empty((B, S), dtype=torch.float32, device=dev)
    L = _lib.lib()
    ws = _workspace(dev, L.dam_masksum_workspace_floats(B, S))
    _lib.check(L.dam_masksum_mse_f32(_lib.ptr(x), _lib.ptr(gains), _lib.ptr(gt), B, S, F * T, _lib.ptr(masked), _lib.ptr(loss),
                                     _lib.ptr(dg), _lib.ptr(ws), _lib.stream()), 'dam_masksum_mse_f32')
    return masked, loss, dg


# ----------------------------------------------------------------------------- optimizer
def adam_l2_step(params, grads, exp_avg, exp_avg_sq, step, derived, lr, beta1, beta2, eps, weight_decay, grad_scale=1.0,
                 hyper=None):
    """hyper: optional CUDA float32[8] {lr, beta1, beta2, eps, weight_decay, grad_scale, 1-beta1, 1-beta2} read by the kernel at run time
    (a captured graph then follows hyper-parameter edits); the scalars are used when it is None."""
    _lib.require_cuda(params, grads, hyper)
    _lib.check(_lib.lib().dam_adam_l2_step_f32(_lib.ptr(params), _lib.ptr(grads), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq),
                                               params.numel(), _lib.ptr(step), _lib.ptr(derived), float(lr), float(beta1),
                                               float(beta2), float(eps), float(weight_decay), float(grad_scale),
                                               _lib.ptr(hyper), _lib.stream()), 'dam_adam_l2_step_f32')


def digest64(t, out=None, index_base=0, accumulate=False, max_blocks=0):
    """Order-independent 64-bit digest of the bit patterns of a contiguous CUDA tensor of 4-byte elements
    (include/dam_hip.h: dam_digest64_u32).  Returns ``out``: a CUDA int64 tensor of one element (the uint64 digest's bits),
    added to when ``accumulate`` -- digest a tensor list piece by piece with index_base = the running element count."""
    _lib.require_cuda(t, out)
    if t.element_size() != 4 or not t.is_contiguous():
        raise ValueError('digest64: a contiguous tensor of 4-byte elements expected (got %s, contiguous=%s)'
                         % (t.dtype, t.is_contiguous()))
    if out is None:
        out = torch.empty(1, dtype=torch.int64, device=t.device)
    elif out.dtype != torch.int64 or out.numel() != 1 or not out.is_contiguous():
        raise ValueError('digest64: out must be a contiguous int64 tensor of one element')
    _lib.check(_lib.lib().dam_digest64_u32(_lib.ptr(t) if t.numel() else None, t.numel(), int(index_base), int(max_blocks),
                                           int(bool(accumulate)), _lib.ptr(out), _lib.stream()), 'dam_digest64_u32')
    return out


# ----------------------------------------------------------------------------- inference tail
def _audio_kind(t, what):
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError('%s must be float32 or float64' % what)
    return 1 if t.dtype == torch.float64 else 0


def gain_ramp_arg(gains, N, n):
    """The optional gain ramps of N tracks of n samples as the batched meters take them: None, or CUDA float64
    [N, n_gains] (or [N]) -> (contiguous [N, n_gains] or None, n_gains or 0)."""
    if gains is None:
        return None, 0
    if gains.dtype != torch.float64:
        raise TypeError('gains must be float64')
    gains = gains.reshape(N, -1).contiguous()
    if not 1 <= gains.shape[1] <= n:
        raise ValueError('between one gain and one gain per sample expected')
    return gains, gains.shape[1]


def gains_smooth(raw_db, window, polyorder=2, out=None, want_f32=False):
    """raw_db: CUDA float32 [n_chunks, S] (model outputs) -> out [2, S, n_chunks] float64 = (10 ** (0.5 * g),
    scipy.signal.savgol_filter(that, window, polyorder) in its default mode 'interp'), computed on the device.
    Returns (amp, smooth[, smooth as float32])."""
    _lib.require_cuda(raw_db, out)
    raw_db = _f32c(raw_db, 'raw_db')
    n, S = raw_db.shape
    if window % 2 == 0 or window <= polyorder or window > n:
        # the conditions scipy.signal.savgol_filter rejects (inference_utils.py:140 would raise there too)
        raise ValueError('savgol_filter needs an odd window with polyorder < window <= len(x): window=%d polyorder=%d '
                         'len=%d' % (window, polyorder, n))
    if out is None:
        out = torch.empty((2, S, n), dtype=torch.float64, device=raw_db.device)
    elif tuple(out.shape) != (2, S, n) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError('bad out tensor')
    s32 = torch.empty((S, n), dtype=torch.float32, device=raw_db.device) if want_f32 else None
    _lib.check(_lib.lib().dam_gains_smooth(_lib.ptr(raw_db), n, S, window, polyorder, _lib.ptr(out[0]), _lib.ptr(out[1]),
                                           _lib.ptr(s32), _lib.stream()), 'dam_gains_smooth')
    return (out[0], out[1], s32) if want_f32 else (out[0], out[1])


def gain_ramp_apply(audio, gains, out=None, out_dtype=None):
    """audio [G, rows_per_gain, n] or [rows, n] (CUDA float32/float64), gains [G, n_gains] or [n_gains] float64 ->
    audio * piecewise-constant gain (one gain sequence per leading index); the result is float64 unless out_dtype says
    float32 (numpy's float32-track * float64-mask product is float64, inference_utils.py:143)."""
    _lib.require_cuda(audio, gains, out)
    ak = _audio_kind(audio, 'audio')
    if gains.dtype != torch.float64:
        raise TypeError('gains must be float64')
    audio, gains = audio.contiguous(), gains.contiguous()
    if audio.dim() == 2:
        rpg, rows, n = audio.shape[0], audio.shape[0], audio.shape[1]
        n_gains = gains.numel()
    else:
        G, rpg, n = audio.shape
        rows, n_gains = G * rpg, gains.shape[-1]
        if gains.numel() != G * n_gains:
            raise ValueError('one gain sequence per leading index expected')
    if out is None:
        out = torch.empty(audio.shape, dtype=out_dtype or torch.float64, device=audio.device)
    elif out.shape != audio.shape or not out.is_contiguous():
        raise ValueError('bad out tensor')
    _lib.check(_lib.lib().dam_gain_ramp_apply(_lib.ptr(audio), ak, _lib.ptr(gains), rows, rpg, n, n_gains, _lib.ptr(out),
                                              _audio_kind(out, 'out'), _lib.stream()), 'dam_gain_ramp_apply')
    return out


def mixdown_peak_normalize(audio, gains, normalize=True, out=None, out_dtype=None, workspace=None):
    """audio [S, rows, n] (CUDA float32/float64), gains [S, n_gains] float64 -> gain-ramped stem sum [rows, n], optionally
    divided row-wise by its max-abs."""
    _lib.require_cuda(audio, gains, out)
    ak = _audio_kind(audio, 'audio')
    if gains.dtype != torch.float64:
        raise TypeError('gains must be float64')
    audio, gains = audio.contiguous(), gains.contiguous()
    S, rows, n = audio.shape
    if out is None:
        out = torch.empty((rows, n), dtype=out_dtype or torch.float64, device=audio.device)
    L = _lib.lib()
    if workspace is None:
        workspace = torch.empty(L.dam_mixdown_workspace_elems(rows), dtype=out.dtype, device=audio.device)
    _lib.check(L.dam_mixdown_peak_normalize(_lib.ptr(audio), ak, _lib.ptr(gains), S, rows, n, gains.shape[1],
                                            1 if normalize else 0, _lib.ptr(out), _audio_kind(out, 'out'),
                                            _lib.ptr(workspace), _lib.stream()), 'dam_mixdown_peak_normalize')
    return out


# ----------------------------------------------------------------------------- PCM encoder (WAV payload)
PCM_FORMATS = {'PCM_16': (0, 2), 'PCM_24': (1, 3), 'PCM_32': (2, 4), 'FLOAT': (3, 4)}    # soundfile's subtype names -> (DAM_WAV_*, bytes)
PCM_MAX_CHANNELS = 8                   # DAM_PCM_MAX_CHANNELS


def pcm_grid_frames(dtype):
    """Frames one pass of the encoder's capped grid covers for float32 / float64 input, asked of the library
    (dam_pcm_tile_frames x dam_pcm_max_blocks): longer buffers are walked tile by tile."""
    L = _lib.lib()
    return L.dam_pcm_tile_frames(1 if dtype in (torch.float64, 'float64') else 0) * L.dam_pcm_max_blocks()


def pcm_encode(x, subtype, scale=None, dither_seed=None, out=None, clip_count=None):
    """x: CUDA float32 / float64 planar [channels, n] (or [n]) -> the interleaved little-endian sample bytes of a WAV `data`
    chunk, uint8 [n * channels * bytes_per_sample] (include/dam_hip.h: dam_pcm_encode).  scale: CUDA float64 of 1 or
    `channels` elements, multiplied in float64 before quantisation.  dither_seed: None = no dither, else the seed of the
    +-1 LSB TPDF dither.  clip_count: CUDA int64 [channels], overwritten with the clamped-sample counts."""
    _lib.require_cuda(x, scale, out, clip_count)
    if subtype not in PCM_FORMATS:
        raise ValueError('pcm_encode: subtype must be one of %s, got %r' % (sorted(PCM_FORMATS), subtype))
    fmt, width = PCM_FORMATS[subtype]
    xk = _audio_kind(x, 'x')
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() != 2 or not x.is_contiguous():
        raise ValueError('pcm_encode: a contiguous [channels, n] tensor expected (got shape %s, contiguous=%s)'
                         % (tuple(x.shape), x.is_contiguous()))
    ch, n = x.shape
    if not 1 <= ch <= PCM_MAX_CHANNELS or n < 1:
        raise ValueError('pcm_encode: 1..%d channels and at least one frame expected, got [%d, %d]' % (PCM_MAX_CHANNELS, ch, n))
    n_scale = 0
    if scale is not None:
        if scale.dtype != torch.float64 or not scale.is_contiguous() or scale.numel() not in (1, ch):
            raise ValueError('pcm_encode: scale must be a contiguous float64 tensor of 1 or %d elements' % ch)
        n_scale = scale.numel()
    if out is None:
        out = torch.empty(n * ch * width, dtype=torch.uint8, device=x.device)
    elif out.dtype != torch.uint8 or out.numel() != n * ch * width or not out.is_contiguous():
        raise ValueError('pcm_encode: out must be a contiguous uint8 tensor of %d elements' % (n * ch * width))
    if clip_count is not None and (clip_count.dtype != torch.int64 or clip_count.numel() != ch or not clip_count.is_contiguous()):
        raise ValueError('pcm_encode: clip_count must be a contiguous int64 tensor of %d elements' % ch)
    seed = 0 if dither_seed is None else int(dither_seed) & 0xFFFFFFFFFFFFFFFF
    _lib.check(_lib.lib().dam_pcm_encode(_lib.ptr(x), xk, ch, n, _lib.ptr(scale), n_scale, fmt,
                                         0 if dither_seed is None else 1, seed, _lib.ptr(out), _lib.ptr(clip_count),
                                         _lib.stream()), 'dam_pcm_encode')
    return out


# ----------------------------------------------------------------------------- true peak and the gain ceiling
def true_peak_geometry():
    """(samples of one workgroup tile, workgroup cap of a launch) of dam_true_peak_batch, asked of the library: a row gets
    max(1, cap // rows) workgroups which stride over its tiles."""
    L = _lib.lib()
    return L.dam_true_peak_tile_samples(), L.dam_true_peak_max_blocks()


def true_peak_batch(data, gains=None, out=None, sample_peak_out=None):
    """data: CUDA float32 / float64 [N, samples, channels] with any strides (planar [N, channels, n] storage is passed as
    ``pcm.transpose(1, 2)``, no copy) -> the linear true peak of every (track, channel) row, float64 [N, channels]
    (include/dam_hip.h: dam_true_peak_batch; 4x oversampled, >= the sample peak).  gains: optional CUDA float64
    [N, n_gains] (or [N]), applied at load exactly as the batched loudness meter applies them.  sample_peak_out: optional
    float64 [N, channels] that receives max |x| of every row.  No host synchronisation, hipGraph-capturable."""
    _lib.require_cuda(data, gains, out, sample_peak_out)
    xk = _audio_kind(data, 'data')
    if data.dim() != 3:
        raise ValueError('true_peak_batch: [tracks, samples, channels] expected, got shape %s' % (tuple(data.shape),))
    N, n, ch = data.shape
    if N < 1 or n < 1 or ch < 1 or N * ch > 65535:
        raise ValueError('true_peak_batch: at least one track, sample and channel and at most 65535 rows expected, got %s'
                         % (tuple(data.shape),))
    gains, n_gains = gain_ramp_arg(gains, N, n)
    dev = data.device
    if out is None:
        out = torch.empty((N, ch), dtype=torch.float64, device=dev)
    for o in (out, sample_peak_out):
        if o is not None and (tuple(o.shape) != (N, ch) or o.dtype != torch.float64 or not o.is_contiguous()):
            raise ValueError('true_peak_batch: outputs must be contiguous float64 [%d, %d] tensors' % (N, ch))
    L = _lib.lib()
    ws = torch.empty(L.dam_true_peak_workspace_bytes(N, n, ch) // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.dam_true_peak_batch(_lib.ptr(data), xk, N, n, ch, data.stride(0), data.stride(1), data.stride(2),
                                         _lib.ptr(gains), n_gains, _lib.ptr(sample_peak_out), _lib.ptr(out), _lib.ptr(ws),
                                         _lib.stream()), 'dam_true_peak_batch')
    return out


def peak_limit_gains(gains, peaks, ceiling_db):
    """gains: CUDA float64 [G], clamped IN PLACE to ``10 ** (ceiling_db / 20) / max(peaks[g])``; peaks: CUDA float64
    [G, peaks_per_gain] (or [G]) linear peaks, e.g. the channels' true peaks of what the gain will scale.  A zero peak
    leaves its gain unchanged.  Returns gains (include/dam_hip.h: dam_peak_limit_gains)."""
    _lib.require_cuda(gains, peaks)
    if gains.dtype != torch.float64 or peaks.dtype != torch.float64 or not gains.is_contiguous():
        raise TypeError('peak_limit_gains: a contiguous float64 gains tensor and float64 peaks expected')
    G = gains.numel()
    if G < 1 or peaks.numel() < G or peaks.numel() % G:
        raise ValueError('peak_limit_gains: %d peaks do not divide among %d gains' % (peaks.numel(), G))
    peaks = peaks.contiguous()
    with torch.cuda.device(gains.device):
        _lib.check(_lib.lib().dam_peak_limit_gains(_lib.ptr(gains), _lib.ptr(peaks), G, peaks.numel() // G,
                                                   float(10.0 ** (float(ceiling_db) / 20.0)), _lib.stream()),
                   'dam_peak_limit_gains')
    return gains


# ----------------------------------------------------------------------------- look-ahead true-peak limiter
def limiter_geometry():
    """(samples one workgroup owns, largest look-ahead, largest hold) of dam_limiter_apply, asked of the library."""
    L = _lib.lib()
    return L.dam_limiter_tile_samples(), L.dam_limiter_max_lookahead(), L.dam_limiter_max_hold()


def limiter_samples(ms, sr):
    """A look-ahead or hold time in milliseconds as samples: max(1, int(ms * sr / 1000 + 0.5))."""
    return max(1, int(float(ms) * sr / 1000.0 + 0.5))


def limiter_apply(data, ceiling_db, lookahead, hold, pre_gain=None, out=None, out_dtype=None, min_gain_out=None,
                  n_limited_out=None, workspace=None):
    """data: CUDA float32 / float64 [N, samples, channels] with any strides (planar [N, channels, n] storage is passed as
    ``pcm.transpose(1, 2)``, no copy): N row sets, the channels of each limited together so that the true peak of
    ``data * pre_gain`` stays at ``ceiling_db`` dBTP (include/dam_hip.h: dam_limiter_apply states the definition).
    lookahead, hold: samples, 1 .. the caps of limiter_geometry() (ValueError beyond them).  pre_gain: optional CUDA float64
    [N], multiplied in before limiting.  Returns (out planar [N, channels, samples] of ``out_dtype`` (float64 unless given),
    min_gain float64 [N], n_limited int64 [N]).  workspace: optional float64 tensor of dam_limiter_workspace_bytes / 8
    elements.  No host synchronisation, hipGraph-capturable."""
    _lib.require_cuda(data, pre_gain, out, min_gain_out, n_limited_out, workspace)
    xk = _audio_kind(data, 'data')
    if data.dim() != 3:
        raise ValueError('limiter_apply: [row sets, samples, channels] expected, got shape %s' % (tuple(data.shape),))
    N, n, ch = data.shape
    if N < 1 or n < 1 or ch < 1 or N > 65535:
        raise ValueError('limiter_apply: 1..65535 row sets and at least one sample and channel expected, got %s'
                         % (tuple(data.shape),))
    L = _lib.lib()
    lookahead, hold = int(lookahead), int(hold)
    if not 1 <= lookahead <= L.dam_limiter_max_lookahead() or not 1 <= hold <= L.dam_limiter_max_hold():
        raise ValueError('limiter_apply: lookahead must be 1..%d samples and hold 1..%d, got %d and %d'
                         % (L.dam_limiter_max_lookahead(), L.dam_limiter_max_hold(), lookahead, hold))
    if pre_gain is not None and (pre_gain.dtype != torch.float64 or pre_gain.numel() != N or not pre_gain.is_contiguous()):
        raise ValueError('limiter_apply: pre_gain must be a contiguous float64 tensor of %d elements' % N)
    dev = data.device
    if out is None:
        out = torch.empty((N, ch, n), dtype=out_dtype or torch.float64, device=dev)
    elif out.numel() != N * ch * n or not out.is_contiguous():
        raise ValueError('limiter_apply: out must be a contiguous tensor of %d x %d x %d elements' % (N, ch, n))
    ok = _audio_kind(out, 'out')
    if min_gain_out is None:
        min_gain_out = torch.empty(N, dtype=torch.float64, device=dev)
    if n_limited_out is None:
        n_limited_out = torch.empty(N, dtype=torch.int64, device=dev)
    for o, dt in ((min_gain_out, torch.float64), (n_limited_out, torch.int64)):
        if o.dtype != dt or o.numel() != N or not o.is_contiguous():
            raise ValueError('limiter_apply: min_gain_out / n_limited_out must be contiguous float64 / int64 tensors of %d' % N)
    need = L.dam_limiter_workspace_bytes(N, n) // 8
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=dev)
    elif workspace.dtype != torch.float64 or workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError('limiter_apply: workspace must be a contiguous float64 tensor of at least %d elements' % need)
    with torch.cuda.device(dev):
        _lib.check(L.dam_limiter_apply(_lib.ptr(data), xk, N, n, ch, data.stride(0), data.stride(1), data.stride(2),
                                       _lib.ptr(pre_gain), float(10.0 ** (float(ceiling_db) / 20.0)), lookahead, hold,
                                       _lib.ptr(out), ok, _lib.ptr(min_gain_out), _lib.ptr(n_limited_out), _lib.ptr(workspace),
                                       _lib.stream()), 'dam_limiter_apply')
    return out, min_gain_out, n_limited_out


# ----------------------------------------------------------------------------- compressor with attack and release
def compressor_geometry():
    """(samples of one chunk, samples one workgroup owns, largest time constant in samples) of dam_compressor_apply, asked of
    the library.  The chunk length is part of the kernel's definition: it fixes the order of every rounding."""
    L = _lib.lib()
    return L.dam_compressor_chunk_samples(), L.dam_compressor_tile_samples(), L.dam_compressor_max_time_samples()


def compressor_constants(threshold_db, knee_db, attack_ms, release_ms, sr, makeup_db=0.0):
    """The four float64 constants dam_compressor_apply takes, computed once, here, so that the kernel and a reference use
    bit-identical values: (knee_start = 10^((T - W/2)/20), alpha_attack = exp(-1 / (attack_ms * 1e-3 * sr)), alpha_release
    likewise, makeup = 10^(makeup_db/20)).  Needs no GPU."""
    import math
    threshold_db, knee_db, attack_ms, release_ms, sr = (float(v) for v in (threshold_db, knee_db, attack_ms, release_ms, sr))
    if not (knee_db >= 0.0 and attack_ms > 0.0 and release_ms > 0.0 and sr > 0.0):
        raise ValueError('compressor_constants: knee_db >= 0 and positive times and rate expected, got %r'
                         % ((knee_db, attack_ms, release_ms, sr),))
    return (10.0 ** ((threshold_db - 0.5 * knee_db) / 20.0), math.exp(-1.0 / (attack_ms * 1e-3 * sr)),
            math.exp(-1.0 / (release_ms * 1e-3 * sr)), 10.0 ** (float(makeup_db) / 20.0))


def compressor_apply(data, threshold_db, ratio, knee_db, knee_start, alpha_attack, alpha_release, makeup=1.0, pre_gain=None,
                     out=None, out_dtype=None, reduction_out=None, max_reduction_out=None, n_over_out=None, workspace=None):
    """data: CUDA float32 / float64 [N, samples, channels] with any strides (planar [N, channels, n] storage is passed as
    ``pcm.transpose(1, 2)``, no copy): N row sets, the channels of each compressed with one gain (include/dam_hip.h:
    dam_compressor_apply states the definition).  threshold_db, ratio (>= 1, ``float('inf')`` allowed), knee_db (>= 0): the
    static curve; knee_start, alpha_attack, alpha_release, makeup: ``compressor_constants(...)`` of the same threshold and
    knee (ValueError where the library refuses them).  pre_gain: optional CUDA float64 [N], multiplied in first.
    reduction_out: optional CUDA float64 [N, samples] that receives the gain-reduction curve in dB.  Returns (out planar
    [N, channels, samples] of ``out_dtype`` (float64 unless given), max_reduction float64 [N] in dB, n_over int64 [N]).
    workspace: optional float64 tensor of dam_compressor_workspace_bytes / 8 elements.  No host synchronisation,
    hipGraph-capturable."""
    _lib.require_cuda(data, pre_gain, out, reduction_out, max_reduction_out, n_over_out, workspace)
    xk = _audio_kind(data, 'data')
    if data.dim() != 3:
        raise ValueError('compressor_apply: [row sets, samples, channels] expected, got shape %s' % (tuple(data.shape),))
    N, n, ch = data.shape
    if N < 1 or n < 1 or ch < 1 or N > 65535:
        raise ValueError('compressor_apply: 1..65535 row sets and at least one sample and channel expected, got %s'
                         % (tuple(data.shape),))
    if pre_gain is not None and (pre_gain.dtype != torch.float64 or pre_gain.numel() != N or not pre_gain.is_contiguous()):
        raise ValueError('compressor_apply: pre_gain must be a contiguous float64 tensor of %d elements' % N)
    L = _lib.lib()
    dev = data.device
    if out is None:
        out = torch.empty((N, ch, n), dtype=out_dtype or torch.float64, device=dev)
    elif out.numel() != N * ch * n or not out.is_contiguous():
        raise ValueError('compressor_apply: out must be a contiguous tensor of %d x %d x %d elements' % (N, ch, n))
    ok = _audio_kind(out, 'out')
    if reduction_out is not None and (reduction_out.dtype != torch.float64 or reduction_out.numel() != N * n
                                      or not reduction_out.is_contiguous()):
        raise ValueError('compressor_apply: reduction_out must be a contiguous float64 tensor of %d x %d elements' % (N, n))
    if max_reduction_out is None:
        max_reduction_out = torch.empty(N, dtype=torch.float64, device=dev)
    if n_over_out is None:
        n_over_out = torch.empty(N, dtype=torch.int64, device=dev)
    for o, dt in ((max_reduction_out, torch.float64), (n_over_out, torch.int64)):
        if o.dtype != dt or o.numel() != N or not o.is_contiguous():
            raise ValueError('compressor_apply: max_reduction_out / n_over_out must be contiguous float64 / int64 tensors of %d' % N)
    need = L.dam_compressor_workspace_bytes(N, n) // 8
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=dev)
    elif workspace.dtype != torch.float64 or workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError('compressor_apply: workspace must be a contiguous float64 tensor of at least %d elements' % need)
    with torch.cuda.device(dev):
        rc = L.dam_compressor_apply(_lib.ptr(data), xk, N, n, ch, data.stride(0), data.stride(1), data.stride(2),
                                    _lib.ptr(pre_gain), float(threshold_db), float(ratio), float(knee_db), float(knee_start),
                                    float(alpha_attack), float(alpha_release), float(makeup), _lib.ptr(out), ok,
                                    _lib.ptr(reduction_out), _lib.ptr(max_reduction_out), _lib.ptr(n_over_out),
                                    _lib.ptr(workspace), _lib.stream())
    if rc == -1:                                       # DAM_ERR_BAD_ARG: everything else was checked above
        raise ValueError('compressor_apply: the library refuses threshold %r dB, ratio %r, knee %r dB with knee_start %r, alphas '
                         '%r / %r, makeup %r' % (threshold_db, ratio, knee_db, knee_start, alpha_attack, alpha_release, makeup))
    _lib.check(rc, 'dam_compressor_apply')
    return out, max_reduction_out, n_over_out


# ----------------------------------------------------------------------------- band spectrum and spectral balance
def spectrum_geometry():
    """(frames one workgroup owns, largest number of bands) of dam_spectrum_band_power, asked of the library."""
    L = _lib.lib()
    return L.dam_spectrum_frames_per_block(), L.dam_spectrum_max_bands()


def spectrum_band_power(data, gains, window, twiddles, n_fft, hop, edges, out=None, workspace=None):
    """data: CUDA float32 / float64 [R, S, samples, channels] with any strides (an expanded leading axis, stride 0, makes
    every mix read the same stems; no copy is made) -> the time-averaged band powers of the R mixes ``sum_s stem_s *
    gains[r, s]``, float64 [R, B] (include/dam_hip.h: dam_spectrum_band_power states the definition).  gains: None (every
    gain exactly 1) or CUDA float64 [R, S, n_gains], applied at load exactly as the batched loudness meter applies them.
    window, twiddles: the float32 tables of features._get_tables for ``n_fft``.  edges: CUDA int32 [B + 1], strictly
    ascending bin edges within 0 .. n_fft/2 + 1 -- their CONTENT cannot be checked here without a copy to the host
    (spectrum.band_power_mix checks the host table it uploads).  workspace: optional float64 tensor of
    dam_spectrum_workspace_bytes / 8 elements.  No host synchronisation, hipGraph-capturable."""
    _lib.require_cuda(data, gains, window, twiddles, edges, out, workspace)
    xk = _audio_kind(data, 'data')
    if data.dim() != 4:
        raise ValueError('spectrum_band_power: [mixes, stems, samples, channels] expected, got shape %s' % (tuple(data.shape),))
    R, S, n, ch = data.shape
    if R < 1 or S < 1 or R > 65535:
        raise ValueError('spectrum_band_power: 1..65535 mixes of at least one stem expected, got %s' % (tuple(data.shape),))
    if ch not in (1, 2):
        raise ValueError('spectrum_band_power: 1 or 2 channels expected, got %d' % ch)
    if not isinstance(n_fft, numbers.Integral) or not isinstance(hop, numbers.Integral):
        raise TypeError('spectrum_band_power: n_fft and hop must be integers')
    n_fft, hop = int(n_fft), int(hop)
    if n_fft < 64 or n_fft > 16384 or n_fft & (n_fft - 1):
        raise ValueError('spectrum_band_power: n_fft must be a power of two from 64 to 16384')
    if hop < 1:
        raise ValueError('spectrum_band_power: hop must be positive')
    if n <= n_fft // 2:
        raise ValueError('spectrum_band_power: reflect padding needs more than n_fft / 2 samples (got %d)' % n)
    gains, n_gains = gain_ramp_arg(gains, R * S, n)
    L = _lib.lib()
    if edges.dtype != torch.int32 or edges.dim() != 1 or not edges.is_contiguous():
        raise TypeError('spectrum_band_power: edges must be a contiguous int32 [bands + 1] tensor')
    B = edges.numel() - 1
    if not 1 <= B <= L.dam_spectrum_max_bands():
        raise ValueError('spectrum_band_power: 1..%d bands expected, got %d' % (L.dam_spectrum_max_bands(), B))
    for t, what, count in ((window, 'window', n_fft), (twiddles, 'twiddles', 2 * n_fft)):
        if t.dtype != torch.float32 or t.numel() != count or not t.is_contiguous():
            raise ValueError('spectrum_band_power: %s must be a contiguous float32 tensor of %d elements' % (what, count))
    dev = data.device
    if out is None:
        out = torch.empty((R, B), dtype=torch.float64, device=dev)
    elif tuple(out.shape) != (R, B) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError('spectrum_band_power: out must be a contiguous float64 [%d, %d] tensor' % (R, B))
    need = L.dam_spectrum_workspace_bytes(R, n, hop, B) // 8
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=dev)
    elif workspace.dtype != torch.float64 or workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError('spectrum_band_power: workspace must be a contiguous float64 tensor of at least %d elements' % need)
    with torch.cuda.device(dev):
        _lib.check(L.dam_spectrum_band_power(_lib.ptr(data), xk, R, S, ch, n, data.stride(0), data.stride(1), data.stride(2),
                                             data.stride(3), _lib.ptr(gains), n_gains, _lib.ptr(window), _lib.ptr(twiddles),
                                             n_fft, hop, _lib.ptr(edges), B, _lib.ptr(out), _lib.ptr(workspace),
                                             _lib.stream()), 'dam_spectrum_band_power')
    return out


def spectrum_balance_error(ref_power, cand_power, err_out=None, n_kept_out=None):
    """ref_power CUDA float64 [B], cand_power [V, B] (or [B]: one candidate) -> (err float64 [V], n_kept int32 [V]): the mean
    absolute difference in dB of the band levels relative to each spectrum's total, over the bands both hold at or above
    -70 dB of their total; NaN where there is none (include/dam_hip.h: dam_spectrum_balance_error)."""
    _lib.require_cuda(ref_power, cand_power, err_out, n_kept_out)
    if cand_power.dim() == 1:
        cand_power = cand_power.unsqueeze(0)
    if ref_power.dtype != torch.float64 or cand_power.dtype != torch.float64:
        raise TypeError('spectrum_balance_error: float64 band powers expected')
    if ref_power.dim() != 1 or cand_power.dim() != 2 or cand_power.shape[1] != ref_power.shape[0]:
        raise ValueError('spectrum_balance_error: [bands] and [variants, bands] expected, got %s and %s'
                         % (tuple(ref_power.shape), tuple(cand_power.shape)))
    ref_power, cand_power = ref_power.contiguous(), cand_power.contiguous()
    V, B = cand_power.shape
    L = _lib.lib()
    if V < 1 or not 1 <= B <= L.dam_spectrum_max_bands():
        raise ValueError('spectrum_balance_error: at least one variant and 1..%d bands expected' % L.dam_spectrum_max_bands())
    dev = ref_power.device
    if err_out is None:
        err_out = torch.empty(V, dtype=torch.float64, device=dev)
    if n_kept_out is None:
        n_kept_out = torch.empty(V, dtype=torch.int32, device=dev)
    for o, dt in ((err_out, torch.float64), (n_kept_out, torch.int32)):
        if o.dtype != dt or o.numel() != V or not o.is_contiguous():
            raise ValueError('spectrum_balance_error: err_out / n_kept_out must be contiguous float64 / int32 tensors of %d' % V)
    with torch.cuda.device(dev):
        _lib.check(L.dam_spectrum_balance_error(_lib.ptr(ref_power), _lib.ptr(cand_power), V, B, _lib.ptr(err_out),
                                                _lib.ptr(n_kept_out), _lib.stream()), 'dam_spectrum_balance_error')
    return err_out, n_kept_out


# ----------------------------------------------------------------------------- gain fit and gain error
GAINFIT_MAX_STEMS = 8                  # DAM_GAINFIT_MAX_STEMS


def gainfit_geometry():
    """(samples of one workgroup tile, largest number of stems) of dam_gainfit_moments; the tile is asked of the library."""
    return _lib.lib().dam_gainfit_tile_samples(), GAINFIT_MAX_STEMS


def gainfit_check_shapes(stems_shape, mix_shape, n_windows):
    """The host-side argument rules of gainfit_moments on shapes alone -> (S, n, channels, W); ValueError / TypeError
    otherwise.  No tensor and no library is touched."""
    if len(stems_shape) != 3:
        raise ValueError('gainfit_moments: stems must be [stems, samples, channels], got shape %s' % (tuple(stems_shape),))
    S, n, ch = stems_shape
    if not 1 <= S <= GAINFIT_MAX_STEMS:
        raise ValueError('gainfit_moments: 1..%d stems expected, got %d' % (GAINFIT_MAX_STEMS, S))
    if ch not in (1, 2):
        raise ValueError('gainfit_moments: 1 or 2 channels expected, got %d' % ch)
    if tuple(mix_shape) != (n, ch):
        raise ValueError('gainfit_moments: the mix must be [samples, channels] = [%d, %d] as the stems are, got shape %s'
                         % (n, ch, tuple(mix_shape)))
    if not isinstance(n_windows, numbers.Integral) or isinstance(n_windows, bool):
        raise TypeError('gainfit_moments: n_windows must be an integer')
    if not 1 <= n_windows <= n:
        raise ValueError('gainfit_moments: between one window and one window per sample expected (%d samples), got %d'
                         % (n, n_windows))
    return S, n, ch, int(n_windows)


def gainfit_check_solve_args(pool, ridge):
    """pool, ridge as gainfit_solve takes them -> (int, float); TypeError / ValueError otherwise."""
    if not isinstance(pool, numbers.Integral) or isinstance(pool, bool):
        raise TypeError('gainfit_solve: pool must be an integer')
    if not isinstance(ridge, numbers.Real) or isinstance(ridge, bool):
        raise TypeError('gainfit_solve: ridge must be a real number')
    if pool < 0 or pool > 0x7fffffff or not float(ridge) >= 0.0:
        raise ValueError('gainfit_solve: pool >= 0 and ridge >= 0 expected, got %r and %r' % (pool, ridge))
    return int(pool), float(ridge)


def gainfit_moments(stems, mix, n_windows, out=None, workspace=None):
    """stems: CUDA float32 / float64 [S, samples, channels] with any strides (planar [S, channels, n] storage is passed as
    ``pcm.transpose(1, 2)``, no copy); mix: CUDA float32 / float64 [samples, channels] with any strides, its dtype
    independent of the stems' -> the moment matrices of (stems, mix) per window, float64 [W, S + 1, S + 1]
    (include/dam_hip.h: dam_gainfit_moments states the definition and the order of the additions).  workspace: optional
    float64 tensor of dam_gainfit_workspace_bytes / 8 elements.  No host synchronisation, hipGraph-capturable."""
    _lib.require_cuda(stems, mix, out, workspace)
    xk, yk = _audio_kind(stems, 'stems'), _audio_kind(mix, 'mix')
    S, n, ch, W = gainfit_check_shapes(stems.shape, mix.shape, n_windows)
    dev = stems.device
    if mix.device != dev:
        raise ValueError('gainfit_moments: the stems and the mix must be on one device')
    if out is None:
        out = torch.empty((W, S + 1, S + 1), dtype=torch.float64, device=dev)
    elif tuple(out.shape) != (W, S + 1, S + 1) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError('gainfit_moments: out must be a contiguous float64 [%d, %d, %d] tensor' % (W, S + 1, S + 1))
    L = _lib.lib()
    need = L.dam_gainfit_workspace_bytes(W, n, S) // 8
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=dev)
    elif workspace.dtype != torch.float64 or workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError('gainfit_moments: workspace must be a contiguous float64 tensor of at least %d elements' % need)
    with torch.cuda.device(dev):
        _lib.check(L.dam_gainfit_moments(_lib.ptr(stems), xk, S, ch, n, stems.stride(0), stems.stride(1), stems.stride(2),
                                         _lib.ptr(mix), yk, mix.stride(0), mix.stride(1), W, _lib.ptr(out),
                                         _lib.ptr(workspace), _lib.stream()), 'dam_gainfit_moments')
    return out


def gainfit_solve(moments, pool=0, ridge=0.0, gains_out=None, residual_out=None, status_out=None):
    """moments: CUDA float64 [W, S + 1, S + 1] (gainfit_moments) -> (gains float64 [S, W], residual float64 [W], status int32
    [W]): the least-squares gains of every window over the moments of windows w - pool .. w + pool, NaN for a stem that is
    silent there (include/dam_hip.h: dam_gainfit_solve).  status: the number of fitted stems, 0 for a silent target, -1 for
    a rank-deficient window (then ``ridge`` > 0 helps)."""
    _lib.require_cuda(moments, gains_out, residual_out, status_out)
    pool, ridge = gainfit_check_solve_args(pool, ridge)
    if moments.dtype != torch.float64:
        raise TypeError('gainfit_solve: float64 moments expected')
    if moments.dim() != 3 or moments.shape[1] != moments.shape[2] or not 2 <= moments.shape[1] <= GAINFIT_MAX_STEMS + 1 \
            or moments.shape[0] < 1:
        raise ValueError('gainfit_solve: moments must be [windows, S + 1, S + 1] with 1..%d stems, got shape %s'
                         % (GAINFIT_MAX_STEMS, tuple(moments.shape)))
    moments = moments.contiguous()
    W, S = moments.shape[0], moments.shape[1] - 1
    dev = moments.device
    if gains_out is None:
        gains_out = torch.empty((S, W), dtype=torch.float64, device=dev)
    if residual_out is None:
        residual_out = torch.empty(W, dtype=torch.float64, device=dev)
    if status_out is None:
        status_out = torch.empty(W, dtype=torch.int32, device=dev)
    for o, dt, shape in ((gains_out, torch.float64, (S, W)), (residual_out, torch.float64, (W,)), (status_out, torch.int32, (W,))):
        if o.dtype != dt or tuple(o.shape) != shape or not o.is_contiguous():
            raise ValueError('gainfit_solve: outputs must be contiguous float64 [%d, %d], float64 [%d] and int32 [%d] tensors'
                             % (S, W, W, W))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dam_gainfit_solve(_lib.ptr(moments), W, S, pool, ridge, _lib.ptr(gains_out),
                                                _lib.ptr(residual_out), _lib.ptr(status_out), _lib.stream()),
                   'dam_gainfit_solve')
    return gains_out, residual_out, status_out


def gainfit_gain_error(fit, cand, err_out=None, err_stem_out=None, n_kept_out=None):
    """fit: CUDA float64 [S, W]; cand: [V, S, W] or [V, S, 1] (a constant gain per stem), or one variant without the leading
    axis -> (err float64 [V], err_stem float64 [V, S], n_kept int32 [V]): the mean over windows and stems of
    |d - the window's mean d|, d = 20 log10(cand / fit), over the entries where both gains are finite and positive and the
    windows that keep at least two stems; NaN where nothing is kept (include/dam_hip.h: dam_gainfit_gain_error)."""
    _lib.require_cuda(fit, cand, err_out, err_stem_out, n_kept_out)
    if cand.dim() == 2:
        cand = cand.unsqueeze(0)
    if fit.dtype != torch.float64 or cand.dtype != torch.float64:
        raise TypeError('gainfit_gain_error: float64 gains expected')
    if fit.dim() != 2 or cand.dim() != 3 or cand.shape[1] != fit.shape[0] or cand.shape[2] not in (1, fit.shape[1]):
        raise ValueError('gainfit_gain_error: [S, W] and [V, S, W or 1] expected, got %s and %s'
                         % (tuple(fit.shape), tuple(cand.shape)))
    S, W = fit.shape
    V, n_cand = cand.shape[0], cand.shape[2]
    if V < 1 or W < 1 or not 1 <= S <= GAINFIT_MAX_STEMS:
        raise ValueError('gainfit_gain_error: at least one variant and window and 1..%d stems expected' % GAINFIT_MAX_STEMS)
    fit, cand = fit.contiguous(), cand.contiguous()
    dev = fit.device
    if err_out is None:
        err_out = torch.empty(V, dtype=torch.float64, device=dev)
    if err_stem_out is None:
        err_stem_out = torch.empty((V, S), dtype=torch.float64, device=dev)
    if n_kept_out is None:
        n_kept_out = torch.empty(V, dtype=torch.int32, device=dev)
    for o, dt, count in ((err_out, torch.float64, V), (err_stem_out, torch.float64, V * S), (n_kept_out, torch.int32, V)):
        if o.dtype != dt or o.numel() != count or not o.is_contiguous():
            raise ValueError('gainfit_gain_error: outputs must be contiguous float64 [%d], float64 [%d, %d] and int32 [%d] tensors'
                             % (V, V, S, V))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dam_gainfit_gain_error(_lib.ptr(fit), _lib.ptr(cand), V, S, W, n_cand, _lib.ptr(err_out),
                                                     _lib.ptr(err_stem_out), _lib.ptr(n_kept_out), _lib.stream()),
                   'dam_gainfit_gain_error')
    return err_out, err_stem_out, n_kept_out


# ----------------------------------------------------------------------------- band gain fit
GAINFIT_BAND_MAX_BANDS = 64            # dam_spectrum_max_bands()


def gainfit_band_frame_windows(n, n_windows, hop):
    """[first frame of window w] for w = 0 .. W (the last entry is the frame count T = 1 + n / hop): window w of the band fit
    owns the frames whose centre sample has gain index w in the mixer's ramp (include/dam_hip.h: Window of a frame)."""
    seg, T = n // n_windows, 1 + n // hop
    return [0] + [min(T, -(-(w * seg) // hop)) for w in range(1, n_windows)] + [T]


def gainfit_band_check_shapes(stems_shape, mix_shape, n_windows, n_fft, hop, n_bands=None):
    """The host-side argument rules of gainfit_band_moments on shapes alone -> (S, n, channels, W, n_fft, hop); ValueError /
    TypeError otherwise.  hop None: n_fft / 2.  No tensor and no library is touched."""
    S, n, ch, W = gainfit_check_shapes(stems_shape, mix_shape, n_windows)
    if not isinstance(n_fft, numbers.Integral) or isinstance(n_fft, bool) or \
            (hop is not None and (not isinstance(hop, numbers.Integral) or isinstance(hop, bool))):
        raise TypeError('gainfit_band_moments: n_fft and hop must be integers')
    n_fft = int(n_fft)
    hop = n_fft // 2 if hop is None else int(hop)
    if n_fft < 64 or n_fft > 16384 or n_fft & (n_fft - 1):
        raise ValueError('gainfit_band_moments: n_fft must be a power of two from 64 to 16384')
    if hop < 1:
        raise ValueError('gainfit_band_moments: hop must be positive')
    if n <= n_fft // 2:
        raise ValueError('gainfit_band_moments: reflect padding needs more than n_fft / 2 samples (got %d)' % n)
    if 1 + n // hop > 0x7fffffff // 2:
        raise ValueError('gainfit_band_moments: too many frames')
    first = gainfit_band_frame_windows(n, W, hop)
    empty = [w for w in range(W) if first[w + 1] <= first[w]]
    if empty:
        raise ValueError('gainfit_band_moments: window %d of %d owns no frame (%d samples, hop %d): fewer windows or a '
                         'smaller hop' % (empty[0], W, n, hop))
    if n_bands is not None and not 1 <= n_bands <= GAINFIT_BAND_MAX_BANDS:
        raise ValueError('gainfit_band_moments: 1..%d bands expected, got %d' % (GAINFIT_BAND_MAX_BANDS, n_bands))
    return S, n, ch, W, n_fft, hop


def gainfit_band_moments(stems, mix, n_windows, window, twiddles, n_fft, hop, edges, out=None, workspace=None, slab_bytes=0):
    """stems, mix as gainfit_moments takes them; window, twiddles: the float32 tables of features._get_tables for ``n_fft``;
    edges: CUDA int32 [B + 1] (content unchecked here, as in spectrum_band_power) -> the moment matrices of (stems, mix) over
    the STFT bins of every band and the frames of every window, float64 [B, W, S + 1, S + 1] (include/dam_hip.h:
    dam_bandfit_moments states the definition and the order of the additions).  slab_bytes: the spectra the workspace
    holds at a time (0: the library's default); it changes no bit of the result.  workspace: optional float64 tensor of
    dam_bandfit_workspace_bytes / 8 elements.  No host synchronisation, hipGraph-capturable."""
    _lib.require_cuda(stems, mix, window, twiddles, edges, out, workspace)
    xk, yk = _audio_kind(stems, 'stems'), _audio_kind(mix, 'mix')
    if edges.dtype != torch.int32 or edges.dim() != 1 or not edges.is_contiguous():
        raise TypeError('gainfit_band_moments: edges must be a contiguous int32 [bands + 1] tensor')
    B = edges.numel() - 1
    S, n, ch, W, n_fft, hop = gainfit_band_check_shapes(stems.shape, mix.shape, n_windows, n_fft, hop, B)
    if not isinstance(slab_bytes, numbers.Integral) or slab_bytes < 0:
        raise ValueError('gainfit_band_moments: slab_bytes must be a non-negative integer')
    for t, what, count in ((window, 'window', n_fft), (twiddles, 'twiddles', 2 * n_fft)):
        if t.dtype != torch.float32 or t.numel() != count or not t.is_contiguous():
            raise ValueError('gainfit_band_moments: %s must be a contiguous float32 tensor of %d elements' % (what, count))
    dev = stems.device
    if mix.device != dev:
        raise ValueError('gainfit_band_moments: the stems and the mix must be on one device')
    shape = (B, W, S + 1, S + 1)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError('gainfit_band_moments: out must be a contiguous float64 %s tensor' % (shape,))
    L = _lib.lib()
    need = L.dam_bandfit_workspace_bytes(W, n, S, ch, n_fft, hop, B, int(slab_bytes))
    if need <= 0:
        raise ValueError('gainfit_band_moments: the library refuses these arguments')
    need = (need + 7) // 8
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=dev)
    elif workspace.dtype != torch.float64 or workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError('gainfit_band_moments: workspace must be a contiguous float64 tensor of at least %d elements' % need)
    with torch.cuda.device(dev):
        _lib.check(L.dam_bandfit_moments(_lib.ptr(stems), xk, S, ch, n, stems.stride(0), stems.stride(1), stems.stride(2),
                                              _lib.ptr(mix), yk, mix.stride(0), mix.stride(1), _lib.ptr(window),
                                              _lib.ptr(twiddles), n_fft, hop, _lib.ptr(edges), B, W, int(slab_bytes),
                                              _lib.ptr(out), _lib.ptr(workspace), _lib.stream()), 'dam_bandfit_moments')
    return out


def gainfit_check_grouped_shape(moments_shape):
    """[G, W, S + 1, S + 1] as gainfit_solve_grouped takes it -> (G, W, S); ValueError otherwise."""
    shape = tuple(moments_shape)
    if len(shape) != 4 or shape[2] != shape[3] or not 2 <= shape[2] <= GAINFIT_MAX_STEMS + 1 or shape[0] < 1 or shape[1] < 1:
        raise ValueError('gainfit_solve_grouped: moments must be [groups, windows, S + 1, S + 1] with 1..%d stems, got shape %s'
                         % (GAINFIT_MAX_STEMS, shape))
    return shape[0], shape[1], shape[2] - 1


def gainfit_solve_grouped(moments, pool=0, ridge=0.0, gains_out=None, residual_out=None, target_out=None, status_out=None):
    """moments: CUDA float64 [G, W, S + 1, S + 1] -> (gains float64 [G, S, W], residual float64 [G, W], target float64 [G, W],
    status int32 [G, W]): gainfit_solve on every group (band) of its own -- windows are pooled within a group only -- and
    ``target``, the mix's energy in the pooled matrix the residual was divided by (include/dam_hip.h:
    dam_bandfit_solve_grouped).  One launch."""
    _lib.require_cuda(moments, gains_out, residual_out, target_out, status_out)
    pool, ridge = gainfit_check_solve_args(pool, ridge)
    if moments.dtype != torch.float64:
        raise TypeError('gainfit_solve_grouped: float64 moments expected')
    G, W, S = gainfit_check_grouped_shape(moments.shape)
    moments = moments.contiguous()
    dev = moments.device
    outs = []
    for o, dt, shape in ((gains_out, torch.float64, (G, S, W)), (residual_out, torch.float64, (G, W)),
                         (target_out, torch.float64, (G, W)), (status_out, torch.int32, (G, W))):
        if o is None:
            o = torch.empty(shape, dtype=dt, device=dev)
        elif o.dtype != dt or tuple(o.shape) != shape or not o.is_contiguous():
            raise ValueError('gainfit_solve_grouped: outputs must be contiguous float64 [%d, %d, %d], float64 [%d, %d] twice and '
                             'int32 [%d, %d] tensors' % (G, S, W, G, W, G, W))
        outs.append(o)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dam_bandfit_solve_grouped(_lib.ptr(moments), G, W, S, pool, ridge, _lib.ptr(outs[0]),
                                                        _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(outs[3]), _lib.stream()),
                   'dam_bandfit_solve_grouped')
    return tuple(outs)


def gainfit_band_summary(residual, target, status, out=None):
    """residual, target CUDA float64 [G, W], status int32 [G, W] (gainfit_solve_grouped) -> total float64 [W]: the share of the
    mix's energy the band-wise gains leave unexplained in every window, NaN where the mix is silent in every band
    (include/dam_hip.h: dam_bandfit_summary)."""
    _lib.require_cuda(residual, target, status, out)
    if residual.dtype != torch.float64 or target.dtype != torch.float64 or status.dtype != torch.int32:
        raise TypeError('gainfit_band_summary: float64 residual and target and int32 status expected')
    if residual.dim() != 2 or residual.shape[0] < 1 or residual.shape[1] < 1 or target.shape != residual.shape \
            or status.shape != residual.shape:
        raise ValueError('gainfit_band_summary: three [groups, windows] tensors expected, got %s, %s and %s'
                         % (tuple(residual.shape), tuple(target.shape), tuple(status.shape)))
    residual, target, status = residual.contiguous(), target.contiguous(), status.contiguous()
    G, W = residual.shape
    if out is None:
        out = torch.empty(W, dtype=torch.float64, device=residual.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (W,) or not out.is_contiguous():
        raise ValueError('gainfit_band_summary: out must be a contiguous float64 [%d] tensor' % W)
    with torch.cuda.device(residual.device):
        _lib.check(_lib.lib().dam_bandfit_summary(_lib.ptr(residual), _lib.ptr(target), _lib.ptr(status), G, W,
                                                       _lib.ptr(out), _lib.stream()), 'dam_bandfit_summary')
    return out


# ----------------------------------------------------------------------------- band-gain mixer
def bandmix_check_shapes(stems_shape, gains_shape, fill_shape, n_fft, hop):
    """The host-side argument rules of bandmix_render on shapes alone -> (S, n, channels, B, W, n_fft, hop); ValueError /
    TypeError otherwise.  stems_shape [S, n, channels]; gains_shape [B, S, W]; fill_shape: () for a number, [S], [S, 1] or
    [S, W]; hop None: n_fft / 2.  No tensor and no library is touched."""
    if len(stems_shape) != 3:
        raise ValueError('bandmix_render: stems must be [stems, samples, channels], got shape %s' % (tuple(stems_shape),))
    S, n, ch = stems_shape
    if not 1 <= S <= GAINFIT_MAX_STEMS:
        raise ValueError('bandmix_render: 1..%d stems expected, got %d' % (GAINFIT_MAX_STEMS, S))
    if ch not in (1, 2):
        raise ValueError('bandmix_render: 1 or 2 channels expected, got %d' % ch)
    if not isinstance(n_fft, numbers.Integral) or isinstance(n_fft, bool) or \
            (hop is not None and (not isinstance(hop, numbers.Integral) or isinstance(hop, bool))):
        raise TypeError('bandmix_render: n_fft and hop must be integers')
    n_fft = int(n_fft)
    hop = n_fft // 2 if hop is None else int(hop)
    if n_fft < 64 or n_fft > 16384 or n_fft & (n_fft - 1):
        raise ValueError('bandmix_render: n_fft must be a power of two from 64 to 16384')
    if not 1 <= hop <= n_fft // 2:
        raise ValueError('bandmix_render: hop must be 1 .. n_fft / 2 (the overlap-add needs every sample under two frames), got %d'
                         % hop)
    if n <= n_fft // 2:
        raise ValueError('bandmix_render: reflect padding needs more than n_fft / 2 samples (got %d)' % n)
    if 1 + n // hop > 0x7fffffff // 2:
        raise ValueError('bandmix_render: too many frames')
    gains_shape = tuple(gains_shape)
    if len(gains_shape) != 3 or gains_shape[1] != S or not 1 <= gains_shape[0] <= GAINFIT_BAND_MAX_BANDS or \
            not 1 <= gains_shape[2] <= n:
        raise ValueError('bandmix_render: gains must be [bands, stems, windows] = [1..%d, %d, 1..%d], got shape %s'
                         % (GAINFIT_BAND_MAX_BANDS, S, n, gains_shape))
    B, W = gains_shape[0], gains_shape[2]
    if tuple(fill_shape) not in ((), (S,), (S, 1), (S, W)):
        raise ValueError('bandmix_render: fill must be a number or [S], [S, 1] or [S, W] = [%d, %d], got shape %s'
                         % (S, W, tuple(fill_shape)))
    first = gainfit_band_frame_windows(n, W, hop)
    empty = [w for w in range(W) if first[w + 1] <= first[w]]
    if empty:
        raise ValueError('bandmix_render: window %d of %d owns no frame (%d samples, hop %d): fewer windows or a smaller hop'
                         % (empty[0], W, n, hop))
    return S, n, ch, B, W, n_fft, hop


def bandmix_render(stems, gains, fill, edges, window, twiddles, n_fft, hop, out=None, workspace=None):
    """stems: CUDA float32 / float64 [S, samples, channels] with any strides; gains: CUDA float64 [B, S, W]; fill: CUDA float64
    [S, W]; edges: CUDA int32 [B + 1] (content unchecked here); window, twiddles: the float32 tables of features._get_tables
    for ``n_fft`` -> the band-gain mix, float32 [channels, samples] (include/dam_hip.h: dam_bandmix_render states the
    definition).  workspace: optional float32 tensor of dam_bandmix_workspace_bytes / 4 elements.  No host synchronisation,
    hipGraph-capturable."""
    _lib.require_cuda(stems, gains, fill, edges, window, twiddles, out, workspace)
    xk = _audio_kind(stems, 'stems')
    if gains.dtype != torch.float64 or fill.dtype != torch.float64:
        raise TypeError('bandmix_render: float64 gains and fill expected')
    if edges.dtype != torch.int32 or edges.dim() != 1 or not edges.is_contiguous():
        raise TypeError('bandmix_render: edges must be a contiguous int32 [bands + 1] tensor')
    S, n, ch, B, W, n_fft, hop = bandmix_check_shapes(stems.shape, gains.shape, fill.shape, n_fft, hop)
    if tuple(fill.shape) != (S, W) or edges.numel() != B + 1:
        raise ValueError('bandmix_render: fill must be [%d, %d] and edges [%d]' % (S, W, B + 1))
    for t, what, count in ((window, 'window', n_fft), (twiddles, 'twiddles', 2 * n_fft)):
        if t.dtype != torch.float32 or t.numel() != count or not t.is_contiguous():
            raise ValueError('bandmix_render: %s must be a contiguous float32 tensor of %d elements' % (what, count))
    dev = stems.device
    if any(t.device != dev for t in (gains, fill, edges, window, twiddles)):
        raise ValueError('bandmix_render: every tensor must be on the stems\' device')
    gains, fill = gains.contiguous(), fill.contiguous()
    if out is None:
        out = torch.empty((ch, n), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (ch, n) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError('bandmix_render: out must be a contiguous float32 [%d, %d] tensor' % (ch, n))
    L = _lib.lib()
    need = L.dam_bandmix_workspace_bytes(n, ch, n_fft, hop)
    if need <= 0:
        raise ValueError('bandmix_render: the library refuses these arguments')
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=dev)
    elif workspace.dtype != torch.float32 or workspace.numel() * 4 < need or not workspace.is_contiguous():
        raise ValueError('bandmix_render: workspace must be a contiguous float32 tensor of at least %d elements' % (need // 4))
    with torch.cuda.device(dev):
        _lib.check(L.dam_bandmix_render(_lib.ptr(stems), xk, S, ch, n, stems.stride(0), stems.stride(1), stems.stride(2),
                                        _lib.ptr(gains), _lib.ptr(fill), _lib.ptr(edges), B, W, _lib.ptr(window),
                                        _lib.ptr(twiddles), n_fft, hop, _lib.ptr(out), _lib.ptr(workspace),
                                        workspace.numel() * 4, _lib.stream()), 'dam_bandmix_render')
    return out


# ----------------------------------------------------------------------------- spectrogram distance
def specdist_check_shapes(stems_shape, gains_shape, ref_shape, ref_gains_shape, n_fft, hop, n_windows, n_bands=None, amin=1e-5):
    """The host-side argument rules of specdist_sums on shapes alone -> (R, S, n, channels, S_ref, ref_channels, n_fft, hop, W);
    ValueError / TypeError otherwise.  stems_shape [S, n, channels]; gains_shape None or [R, S, n_gains]; ref_shape
    [S_ref, n, channels]; ref_gains_shape None or [S_ref, n_gains]; hop None: n_fft / 2.  No tensor and no library is touched."""
    if len(stems_shape) != 3 or len(ref_shape) != 3:
        raise ValueError('specdist_sums: stems and reference must be [stems, samples, channels], got shapes %s and %s'
                         % (tuple(stems_shape), tuple(ref_shape)))
    S, n, ch = stems_shape
    S_ref, n_ref, ch_ref = ref_shape
    if S < 1 or S_ref < 1:
        raise ValueError('specdist_sums: at least one stem on either side expected')
    if ch not in (1, 2) or ch_ref not in (1, 2):
        raise ValueError('specdist_sums: 1 or 2 channels expected, got %d and %d' % (ch, ch_ref))
    if n_ref != n:
        raise ValueError('specdist_sums: the reference has %d samples, the stems %d: equal lengths expected' % (n_ref, n))
    for v in (n_fft, n_windows) + (() if hop is None else (hop,)):
        if not isinstance(v, numbers.Integral) or isinstance(v, bool):
            raise TypeError('specdist_sums: n_fft, hop and n_windows must be integers')
    n_fft, W = int(n_fft), int(n_windows)
    hop = n_fft // 2 if hop is None else int(hop)
    if n_fft < 64 or n_fft > 16384 or n_fft & (n_fft - 1):
        raise ValueError('specdist_sums: n_fft must be a power of two from 64 to 16384')
    if hop < 1:
        raise ValueError('specdist_sums: hop must be positive')
    if n <= n_fft // 2:
        raise ValueError('specdist_sums: reflect padding needs more than n_fft / 2 samples (got %d)' % n)
    if 1 + n // hop > 0x7fffffff // 2:
        raise ValueError('specdist_sums: too many frames')
    R = 1
    if gains_shape is not None:
        gains_shape = tuple(gains_shape)
        if len(gains_shape) != 3 or gains_shape[1] != S or not 1 <= gains_shape[0] <= 65535 or not 1 <= gains_shape[2] <= n:
            raise ValueError('specdist_sums: gains must be [rows, stems, n_gains] = [1..65535, %d, 1..%d], got shape %s'
                             % (S, n, gains_shape))
        R = gains_shape[0]
    if ref_gains_shape is not None:
        ref_gains_shape = tuple(ref_gains_shape)
        if len(ref_gains_shape) != 2 or ref_gains_shape[0] != S_ref or not 1 <= ref_gains_shape[1] <= n:
            raise ValueError('specdist_sums: ref_gains must be [stems, n_gains] = [%d, 1..%d], got shape %s'
                             % (S_ref, n, ref_gains_shape))
    if not 1 <= W <= n:
        raise ValueError('specdist_sums: 1..%d windows expected, got %d' % (n, W))
    first = gainfit_band_frame_windows(n, W, hop) if W <= 1 + n // hop else None
    empty = [0] if first is None else [w for w in range(W) if first[w + 1] <= first[w]]
    if empty:
        raise ValueError('specdist_sums: window %d of %d owns no frame (%d samples, hop %d): fewer windows or a smaller hop'
                         % (empty[0], W, n, hop))
    if n_bands is not None and not 1 <= n_bands <= GAINFIT_BAND_MAX_BANDS:
        raise ValueError('specdist_sums: 1..%d bands expected, got %d' % (GAINFIT_BAND_MAX_BANDS, n_bands))
    if not isinstance(amin, numbers.Real) or isinstance(amin, bool) or not float(amin) > 0.0 or \
            not ctypes.c_float(float(amin)).value > 0.0:
        raise ValueError('specdist_sums: amin must be a positive float32 number')
    return R, S, n, ch, S_ref, ch_ref, n_fft, hop, W


def specdist_sums(stems, gains, ref_stems, ref_gains, window, twiddles, n_fft, hop, edges, n_windows, amin=1e-5, sums_out=None,
                  count_out=None, workspace=None):
    """stems: CUDA float32 / float64 [S, samples, channels] with any strides; gains: None (one row, the plain sum) or CUDA float64
    [R, S, n_gains]; ref_stems: CUDA float32 / float64 [S_ref, samples, channels], the reference mix as its own stems;
    ref_gains: None or CUDA float64 [S_ref, n_gains]; window, twiddles: the float32 tables of features._get_tables for
    ``n_fft``; edges: CUDA int32 [B + 1] (content unchecked here, as in spectrum_band_power) -> (sums float64 [R, B, W, 2],
    count int64 [B, W]): (sum d, sum d^2) of the dB-spectrogram difference of every row against the reference over the bins
    of band b and the frames of window w, and the number of (frame, bin) pairs in the cell (include/dam_hip.h:
    dam_specdist_sums states the definition and the order of the additions).  workspace: optional float64 tensor of
    dam_specdist_workspace_bytes / 8 elements.  No host synchronisation, hipGraph-capturable."""
    _lib.require_cuda(stems, gains, ref_stems, ref_gains, window, twiddles, edges, sums_out, count_out, workspace)
    xk, rk = _audio_kind(stems, 'stems'), _audio_kind(ref_stems, 'ref_stems')
    for g, what in ((gains, 'gains'), (ref_gains, 'ref_gains')):
        if g is not None and g.dtype != torch.float64:
            raise TypeError('specdist_sums: %s must be float64' % what)
    if edges.dtype != torch.int32 or edges.dim() != 1 or not edges.is_contiguous():
        raise TypeError('specdist_sums: edges must be a contiguous int32 [bands + 1] tensor')
    B = edges.numel() - 1
    R, S, n, ch, S_ref, ch_ref, n_fft, hop, W = specdist_check_shapes(
        stems.shape, None if gains is None else gains.shape, ref_stems.shape, None if ref_gains is None else ref_gains.shape,
        n_fft, hop, n_windows, B, amin)
    for t, what, count in ((window, 'window', n_fft), (twiddles, 'twiddles', 2 * n_fft)):
        if t.dtype != torch.float32 or t.numel() != count or not t.is_contiguous():
            raise ValueError('specdist_sums: %s must be a contiguous float32 tensor of %d elements' % (what, count))
    dev = stems.device
    if any(t is not None and t.device != dev for t in (gains, ref_stems, ref_gains, edges, window, twiddles)):
        raise ValueError('specdist_sums: every tensor must be on the stems\' device')
    gains = None if gains is None else gains.contiguous()
    ref_gains = None if ref_gains is None else ref_gains.contiguous()
    outs = []
    for o, dt, shape in ((sums_out, torch.float64, (R, B, W, 2)), (count_out, torch.int64, (B, W))):
        if o is None:
            o = torch.empty(shape, dtype=dt, device=dev)
        elif o.dtype != dt or tuple(o.shape) != shape or not o.is_contiguous():
            raise ValueError('specdist_sums: outputs must be contiguous float64 %s and int64 %s tensors'
                             % ((R, B, W, 2), (B, W)))
        outs.append(o)
    L = _lib.lib()
    need = L.dam_specdist_workspace_bytes(R, n, n_fft, hop, B, W)
    if need <= 0:
        raise ValueError('specdist_sums: the library refuses these arguments')
    if workspace is None:
        workspace = torch.empty(need // 8, dtype=torch.float64, device=dev)
    elif workspace.dtype != torch.float64 or workspace.numel() * 8 < need or not workspace.is_contiguous() or \
            workspace.data_ptr() % 16:
        raise ValueError('specdist_sums: workspace must be a contiguous, 16-byte aligned float64 tensor of at least %d elements'
                         % (need // 8))
    with torch.cuda.device(dev):
        _lib.check(L.dam_specdist_sums(_lib.ptr(stems), xk, R, S, ch, n, stems.stride(0), stems.stride(1), stems.stride(2),
                                       _lib.ptr(gains), 0 if gains is None else gains.shape[2], _lib.ptr(ref_stems), rk, S_ref,
                                       ch_ref, ref_stems.stride(0), ref_stems.stride(1), ref_stems.stride(2), _lib.ptr(ref_gains),
                                       0 if ref_gains is None else ref_gains.shape[1], _lib.ptr(window), _lib.ptr(twiddles),
                                       n_fft, hop, float(amin), _lib.ptr(edges), B, W, _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                                       _lib.ptr(workspace), _lib.stream()), 'dam_specdist_sums')
    return outs[0], outs[1]


def specdist_summary(sums, count, out=None):
    """sums CUDA float64 [R, B, W, 2], count int64 [B, W] (specdist_sums) -> float64 [R, 1 + B + W, 3]: (mse in dB^2, bias in
    dB, centred rms in dB) of every row as a whole (index 0), per band (1 + b) and per window (1 + B + w); NaN where the
    count is 0 (include/dam_hip.h: dam_specdist_summary).  One launch, nothing comes to the host."""
    _lib.require_cuda(sums, count, out)
    if sums.dtype != torch.float64 or count.dtype != torch.int64:
        raise TypeError('specdist_summary: float64 sums and int64 count expected')
    if sums.dim() != 4 or sums.shape[3] != 2 or count.dim() != 2 or tuple(count.shape) != tuple(sums.shape[1:3]) or \
            sums.shape[0] < 1 or not 1 <= sums.shape[1] <= GAINFIT_BAND_MAX_BANDS or sums.shape[2] < 1:
        raise ValueError('specdist_summary: [rows, bands, windows, 2] with 1..%d bands and [bands, windows] expected, got %s and %s'
                         % (GAINFIT_BAND_MAX_BANDS, tuple(sums.shape), tuple(count.shape)))
    if count.device != sums.device:
        raise ValueError('specdist_summary: the sums and the count must be on one device')
    sums, count = sums.contiguous(), count.contiguous()
    R, B, W = sums.shape[:3]
    shape = (R, 1 + B + W, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=sums.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError('specdist_summary: out must be a contiguous float64 %s tensor' % (shape,))
    with torch.cuda.device(sums.device):
        _lib.check(_lib.lib().dam_specdist_summary(_lib.ptr(sums), _lib.ptr(count), R, B, W, _lib.ptr(out), _lib.stream()),
                   'dam_specdist_summary')
    return out


# ----------------------------------------------------------------------------- spectrogram distance: gradient in the gains
def specgrad_check_shapes(stems_shape, gains_shape, ref_shape, ref_gains_shape, n_fft, hop, amin=1e-5):
    """The host-side argument rules of specgrad on shapes alone -> (clips, R, S, n, channels, S_ref, ref_channels, n_fft, hop,
    n_gains); ValueError / TypeError otherwise.  stems_shape [clips, S, n, channels]; gains_shape None or [clips, R, S, n_gains];
    ref_shape [clips, S_ref, n, channels]; ref_gains_shape None or [clips, S_ref, n_gains]; hop None: n_fft / 2.  n_gains comes
    back as 1 for gains_shape None.  A frame may touch two gain segments at most: n_gains == 1 or n // n_gains >= n_fft.  No
    tensor and no library is touched."""
    if len(stems_shape) != 4 or len(ref_shape) != 4:
        raise ValueError('specgrad: stems and reference must be [clips, stems, samples, channels], got shapes %s and %s'
                         % (tuple(stems_shape), tuple(ref_shape)))
    clips = stems_shape[0]
    if not 1 <= clips <= 65535 or ref_shape[0] != clips:
        raise ValueError('specgrad: 1..65535 clips on both sides expected, got %d and %d' % (clips, ref_shape[0]))
    if gains_shape is not None:
        gains_shape = tuple(gains_shape)
        if len(gains_shape) != 4 or gains_shape[0] != clips:
            raise ValueError('specgrad: gains must be [clips, rows, stems, n_gains] with %d clips, got shape %s' % (clips, gains_shape))
    if ref_gains_shape is not None:
        ref_gains_shape = tuple(ref_gains_shape)
        if len(ref_gains_shape) != 3 or ref_gains_shape[0] != clips:
            raise ValueError('specgrad: ref_gains must be [clips, stems, n_gains] with %d clips, got shape %s'
                             % (clips, ref_gains_shape))
    # the per-clip rules are the distance's (one window: every geometry has a frame)
    R, S, n, ch, S_ref, ch_ref, n_fft, hop, _ = specdist_check_shapes(
        tuple(stems_shape)[1:], None if gains_shape is None else gains_shape[1:], tuple(ref_shape)[1:],
        None if ref_gains_shape is None else ref_gains_shape[1:], n_fft, hop, 1, None, amin)
    G = 1 if gains_shape is None else gains_shape[3]
    if G > 1 and n // G < n_fft:
        raise ValueError('specgrad: unsupported gain ramp: %d samples per gain node, fewer than n_fft = %d (a frame may touch two '
                         'gain segments at most)' % (n // G, n_fft))
    return clips, R, S, n, ch, S_ref, ch_ref, n_fft, hop, G


def specgrad(stems, gains, ref_stems, ref_gains, window, twiddles, n_fft, hop, amin=1e-5, value_out=None, grad_out=None,
             workspace=None):
    """stems: CUDA float32 / float64 [clips, S, samples, channels] with any strides; gains: None (one row, every gain 1) or CUDA
    float64 [clips, R, S, n_gains]; ref_stems: CUDA float32 / float64 [clips, S_ref, samples, channels]; ref_gains: None or CUDA
    float64 [clips, S_ref, n_gains]; window, twiddles: the float32 tables of features._get_tables for ``n_fft`` ->
    (value float64 [clips, R, 2] = (sum d, sum d^2) over every frame and bin, grad float64 [clips, R, S, n_gains] = the gradient
    of sum d^2 in the gains; n_gains 1 for gains None) (include/dam_hip.h: dam_specgrad states the definition and the order of
    the additions).  workspace: optional float64 tensor of dam_specgrad_workspace_bytes / 8 elements.  No host
    synchronisation, hipGraph-capturable."""
    _lib.require_cuda(stems, gains, ref_stems, ref_gains, window, twiddles, value_out, grad_out, workspace)
    xk, rk = _audio_kind(stems, 'stems'), _audio_kind(ref_stems, 'ref_stems')
    for g, what in ((gains, 'gains'), (ref_gains, 'ref_gains')):
        if g is not None and g.dtype != torch.float64:
            raise TypeError('specgrad: %s must be float64' % what)
    clips, R, S, n, ch, S_ref, ch_ref, n_fft, hop, G = specgrad_check_shapes(
        stems.shape, None if gains is None else gains.shape, ref_stems.shape, None if ref_gains is None else ref_gains.shape,
        n_fft, hop, amin)
    for t, what, count in ((window, 'window', n_fft), (twiddles, 'twiddles', 2 * n_fft)):
        if t.dtype != torch.float32 or t.numel() != count or not t.is_contiguous():
            raise ValueError('specgrad: %s must be a contiguous float32 tensor of %d elements' % (what, count))
    dev = stems.device
    if any(t is not None and t.device != dev for t in (gains, ref_stems, ref_gains, window, twiddles)):
        raise ValueError('specgrad: every tensor must be on the stems\' device')
    gains = None if gains is None else gains.contiguous()
    ref_gains = None if ref_gains is None else ref_gains.contiguous()
    outs = []
    for o, shape in ((value_out, (clips, R, 2)), (grad_out, (clips, R, S, G))):
        if o is None:
            o = torch.empty(shape, dtype=torch.float64, device=dev)
        elif o.dtype != torch.float64 or tuple(o.shape) != shape or not o.is_contiguous():
            raise ValueError('specgrad: outputs must be contiguous float64 %s and %s tensors' % ((clips, R, 2), (clips, R, S, G)))
        outs.append(o)
    L = _lib.lib()
    need = L.dam_specgrad_workspace_bytes(clips, R, S, n, n_fft, hop, 0 if gains is None else G)
    if need <= 0:
        raise ValueError('specgrad: the library refuses these arguments')
    if workspace is None:
        workspace = torch.empty(need // 8, dtype=torch.float64, device=dev)
    elif workspace.dtype != torch.float64 or workspace.numel() * 8 < need or not workspace.is_contiguous() or \
            workspace.data_ptr() % 16:
        raise ValueError('specgrad: workspace must be a contiguous, 16-byte aligned float64 tensor of at least %d elements'
                         % (need // 8))
    with torch.cuda.device(dev):
        _lib.check(L.dam_specgrad(_lib.ptr(stems), xk, clips, R, S, ch, n, stems.stride(0), stems.stride(1), stems.stride(2),
                                  stems.stride(3), _lib.ptr(gains), 0 if gains is None else G, _lib.ptr(ref_stems), rk, S_ref,
                                  ch_ref, ref_stems.stride(0), ref_stems.stride(1), ref_stems.stride(2), ref_stems.stride(3),
                                  _lib.ptr(ref_gains), 0 if ref_gains is None else ref_gains.shape[2], _lib.ptr(window),
                                  _lib.ptr(twiddles), n_fft, hop, float(amin), _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                                  _lib.ptr(workspace), _lib.stream()), 'dam_specgrad')
    return outs[0], outs[1]


# ----------------------------------------------------------------------------- alignment
ALIGN_MAX_STEMS = 8
ALIGN_WEIGHTINGS = {'plain': 0, 'phat': 1}      # DAM_ALIGN_PLAIN, DAM_ALIGN_PHAT
ALIGN_MAX_LAG = 4096                            # dam_align_max_lag(); align_geometry() asks the library


def align_geometry(max_lag=None):
    """(largest max_lag, frames one workgroup owns) of dam_align_estimate, asked of the library; with ``max_lag`` also the
    frame length N and the hop H = N / 2 for it: (cap, F, N, H)."""
    L = _lib.lib()
    cap, F = L.dam_align_max_lag(), L.dam_align_frames_per_block()
    if max_lag is None:
        return cap, F
    N = L.dam_align_fft_size(int(max_lag))
    if N <= 0:
        raise ValueError('align: max_lag must be 1..%d, got %r' % (cap, max_lag))
    return cap, F, N, N // 2


def align_check_shapes(stems_shape, mix_shape, max_lag, weighting='phat'):
    """The host-side argument rules of align_estimate on shapes alone -> (S, n, channels, L, weighting code); ValueError /
    TypeError otherwise.  No tensor and no library is touched."""
    if len(stems_shape) != 3:
        raise ValueError('align: stems must be [stems, samples, channels], got shape %s' % (tuple(stems_shape),))
    S, n, ch = stems_shape
    if not 1 <= S <= ALIGN_MAX_STEMS:
        raise ValueError('align: 1..%d stems expected, got %d' % (ALIGN_MAX_STEMS, S))
    if ch not in (1, 2):
        raise ValueError('align: 1 or 2 channels expected, got %d' % ch)
    if n < 1:
        raise ValueError('align: at least one sample expected')
    if mix_shape is not None and tuple(mix_shape) != (n, ch):
        raise ValueError('align: the mix must be [samples, channels] = [%d, %d] as the stems are, got shape %s'
                         % (n, ch, tuple(mix_shape)))
    if not isinstance(max_lag, numbers.Integral) or isinstance(max_lag, bool):
        raise TypeError('align: max_lag must be an integer')
    if not 1 <= max_lag <= ALIGN_MAX_LAG:
        raise ValueError('align: max_lag must be 1..%d samples, got %d' % (ALIGN_MAX_LAG, max_lag))
    if weighting not in ALIGN_WEIGHTINGS:
        raise ValueError('align: unknown weighting %r (expected one of %s)' % (weighting, sorted(ALIGN_WEIGHTINGS)))
    return S, n, ch, int(max_lag), ALIGN_WEIGHTINGS[weighting]


def align_estimate(stems, mix, max_lag, weighting='phat', twiddles=None, want_curve=False, workspace=None):
    """stems: CUDA float32 / float64 [S, samples, channels] with any strides; mix: CUDA float32 / float64 [samples, channels]
    with any strides, its dtype independent of the stems' -> (lag int32 [S], frac float64 [S], peak float64 [S], sign int32
    [S], status int32 [S], curve float64 [S, 2 max_lag + 1] or None): the lag of the largest |cross-correlation| of every stem
    with the mix within +-max_lag samples (include/dam_hip.h: dam_align_estimate states the definitions and the order of the
    additions).  twiddles: the float32 table of features._get_tables for dam_align_fft_size(max_lag), fetched when None.
    workspace: optional float64 tensor of dam_align_workspace_bytes / 8 elements.  No host synchronisation,
    hipGraph-capturable (once the table is resident: a first call outside the capture uploads it)."""
    _lib.require_cuda(stems, mix, twiddles, workspace)
    xk, yk = _audio_kind(stems, 'stems'), _audio_kind(mix, 'mix')
    S, n, ch, Lg, wcode = align_check_shapes(stems.shape, mix.shape, max_lag, weighting)
    dev = stems.device
    if mix.device != dev:
        raise ValueError('align_estimate: the stems and the mix must be on one device')
    L = _lib.lib()
    N = L.dam_align_fft_size(Lg)
    if twiddles is None:
        from . import features
        twiddles = features._get_tables(dev, N)[1]
    if twiddles.dtype != torch.float32 or twiddles.numel() != 2 * N or not twiddles.is_contiguous():
        raise ValueError('align_estimate: twiddles must be a contiguous float32 tensor of %d elements' % (2 * N))
    need = L.dam_align_workspace_bytes(S, n, Lg) // 8
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float64, device=dev)
    elif workspace.dtype != torch.float64 or workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError('align_estimate: workspace must be a contiguous float64 tensor of at least %d elements' % need)
    lag = torch.empty(S, dtype=torch.int32, device=dev)
    sign = torch.empty(S, dtype=torch.int32, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    frac = torch.empty(S, dtype=torch.float64, device=dev)
    peak = torch.empty(S, dtype=torch.float64, device=dev)
    curve = torch.empty((S, 2 * Lg + 1), dtype=torch.float64, device=dev) if want_curve else None
    with torch.cuda.device(dev):
        _lib.check(L.dam_align_estimate(_lib.ptr(stems), xk, S, ch, n, stems.stride(0), stems.stride(1), stems.stride(2),
                                        _lib.ptr(mix), yk, mix.stride(0), mix.stride(1), Lg, wcode, _lib.ptr(twiddles),
                                        _lib.ptr(lag), _lib.ptr(frac), _lib.ptr(peak), _lib.ptr(sign), _lib.ptr(status),
                                        _lib.ptr(curve), _lib.ptr(workspace), _lib.stream()), 'dam_align_estimate')
    return lag, frac, peak, sign, status, curve


def align_shift(stems, lag, out=None):
    """stems: CUDA float32 / float64 [S, samples, channels] with any strides; lag: CUDA int32 [S] (read on the device) ->
    out[s, p] = stems[s, p - lag[s]], 0 outside the stem: the stems' dtype, and their layout where that is dense (planar
    storage stays planar), contiguous otherwise.  out: optional tensor of that shape and dtype that does not overlap the
    stems.  No host synchronisation, hipGraph-capturable."""
    _lib.require_cuda(stems, lag, out)
    xk = _audio_kind(stems, 'stems')
    S, n, ch, _, _ = align_check_shapes(stems.shape, None, 1)
    if lag.dtype != torch.int32 or tuple(lag.shape) != (S,) or not lag.is_contiguous():
        raise ValueError('align_shift: lag must be a contiguous int32 [%d] tensor' % S)
    if lag.device != stems.device:
        raise ValueError('align_shift: the stems and the lags must be on one device')
    if out is None:
        if stems.transpose(1, 2).is_contiguous():
            out = torch.empty((S, ch, n), dtype=stems.dtype, device=stems.device).transpose(1, 2)
        else:
            out = torch.empty((S, n, ch), dtype=stems.dtype, device=stems.device)
    elif tuple(out.shape) != (S, n, ch) or out.dtype != stems.dtype or out.device != stems.device:
        raise ValueError('align_shift: out must be a %s [%d, %d, %d] tensor on the stems\' device' % (stems.dtype, S, n, ch))
    with torch.cuda.device(stems.device):
        _lib.check(_lib.lib().dam_align_shift(_lib.ptr(stems), xk, S, ch, n, stems.stride(0), stems.stride(1), stems.stride(2),
                                              _lib.ptr(lag), _lib.ptr(out), out.stride(0), out.stride(1), out.stride(2),
                                              _lib.stream()), 'dam_align_shift')
    return out


# ----------------------------------------------------------------------------- dropout
_dropout_counters = {}


def _dropout_counter(device):
    device = torch.device(device)
    key = (device.type, torch.cuda.current_device() if device.index is None else device.index)
    if key not in _dropout_counters:
        _dropout_counters[key] = torch.zeros(1, dtype=torch.int64, device=device)
    return _dropout_counters[key]


def dropout_counter(device):
    """The per-device dropout call counter as a Python int (synchronises): the offset the next dropout call will use."""
    return int(_dropout_counter(device).item())


def set_dropout_counter(device, value):
    """Sets the per-device dropout call counter (in stream order): resuming a run at a known offset, and the tests."""
    _dropout_counter(device).fill_(int(value))


def dropout_check(n, p):
    """The argument checks of dam_dropout_apply_f32, for callers that must know BEFORE they advance the counter."""
    if n <= 0 or n % 4:
        raise ValueError('dropout: the element count must be a positive multiple of 4, got %d' % n)
    if not 0.0 <= p < 1.0:
        raise ValueError('dropout: p must lie in [0, 1), got %r' % (p,))


def dropout_tick(device, n):
    """Snapshots and advances the per-device dropout call counter; returns the snapshot tensor (int64[1])."""
    counter = _dropout_counter(device)
    snap = torch.empty(1, dtype=torch.int64, device=device)
    _lib.check(_lib.lib().dam_dropout_tick(_lib.ptr(counter), n, _lib.ptr(snap), _lib.stream()), 'dam_dropout_tick')
    return snap


def dropout_apply(x, p, seed, snapshot):
    _lib.require_cuda(x, snapshot)
    x = x.contiguous()
    y = torch.empty_like(x)
    _lib.check(_lib.lib().dam_dropout_apply_f32(_lib.ptr(x), x.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(snapshot),
                                                _lib.ptr(y), _lib.stream()), 'dam_dropout_apply_f32')
    return y
