"""Test-side wrappers around the single-kernel C-ABI entry points of libr2dm_hip.so."""
import contextlib
import ctypes
import os

import torch

from r2dm_amd import _lib


def _st(t):
    return _lib.stream_ptr(t.device)


@contextlib.contextmanager
def env(**kv):
    """Environment switches for the duration of a block (the library reads most of them per call); a value of None leaves its name alone.
    On exit every name is what it was before: its previous value, or unset."""
    kv = {k: str(v) for k, v in kv.items() if v is not None}
    saved = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def set_conv_pieces(n):
    """Operand split of the single-kernel conv entry: 2 = fp16 + scaled fp16 residual where the shape allows (default),
    3 = three bf16 pieces."""
    _lib.check(_lib.lib().r2dm_set_conv_pieces(None, n))


def conv2d_ring(x, w, b, aff=None, prologue=0, residual=None, scale=None, io16=0):
    """io16 (with R2DM_TEST_IO16 set to the same value by the caller): bit 0 -- x is a half tensor, bit 1 -- the residual is and y will be."""
    L = _lib.lib()
    B, cin, H, W = x.shape
    cout, k = w.shape[0], w.shape[-1]
    w, b = _lib.f32c(w), _lib.f32c(b)
    x = x.detach().half().contiguous() if io16 & 1 else _lib.f32c(x)
    if residual is not None:
        residual = residual.detach().half().contiguous() if io16 & 2 else _lib.f32c(residual)
    packed = torch.empty(L.r2dm_conv_packed_elems(cout, cin, k, B, H, W), device=x.device)
    y = torch.empty(B, cout, H, W, device=x.device, dtype=torch.float16 if io16 & 2 else torch.float32)
    sc = None if scale is None else torch.tensor([scale], device=x.device, dtype=torch.float32)
    _lib.check(L.r2dm_conv2d_ring(x.data_ptr(), w.data_ptr(), b.data_ptr(), packed.data_ptr(), _lib.ptr(aff), prologue,
                                  _lib.ptr(residual), _lib.ptr(sc), y.data_ptr(), B, cin, cout, H, W, k, _st(x)))
    torch.cuda.synchronize()
    return y


def guarded(shape, dtype, guard, device, fill=float("nan")):
    """(whole, view): a `fill`-filled flat buffer and the contiguous view of `shape` in its middle, `guard` elements from either end."""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((guard + n + guard,), fill, device=device, dtype=dtype)
    return whole, whole[guard:guard + n].view(*shape)


def guard_intact(whole, guard, fill=float("nan")):
    """The two bands around a guarded() view still hold their fill (NaN by default)."""
    return fill_intact(whole[:guard], fill) and fill_intact(whole[-guard:], fill)


def fill_intact(t, fill):
    return bool(torch.isnan(t).all() if fill != fill else (t == fill).all())


Y16_CANARY = -60000.0  # the finite fill of a half output and its guard bands: an fp16 number that no test's output reaches


class ConvExResult:
    """y; stat (B, groups, slots, 2) float64 or None; range: the int32[2] record after the call (CPU) or None; chosen: (algo, co_tile, px_rows)."""

    def __init__(self, y, stat, range_, chosen):
        self.y, self.stat, self.range, self.chosen = y, stat, range_, chosen


ALGO_F32, ALGO_BF16X3, ALGO_DIRECT, ALGO_F16X2, ALGO_P1F16 = range(5)  # ConvAlgo (csrc/common.h), as r2dm_conv2d_ring_ex reports it


def conv2d_ring_ex(x, w, b, x1=None, aff=None, prologue=0, residual=None, res_broadcast=False, scale=None, stat_groups=0, stat_goff=0, stat_cpg=0,
                   range_init=None, reverse=0, c1=None, io16=0):
    """r2dm_conv2d_ring_ex: x1 -- the last channels of the input in a second allocation (x holds the first ones; c1 overrides x1's channel
    count, for the refusal tests); stat_groups > 0 -- a statistics sink of that many groups; range_init -- the two int32 the range record
    starts from (None: no record).  y and the sink start NaN-filled inside NaN guard bands (one plane / 64 doubles) that must survive the
    call; if the entry refuses, y, the sink and the packed-weight buffer (NaN-filled too) must still hold nothing but the fill, and the error
    is raised on.
    io16 (with R2DM_TEST_IO16 set to the same value by the caller, as for conv2d_ring): bit 0 -- x and x1 are half tensors (passed as they are
    if they are already: a guarded view stays where it is), bit 1 -- the residual is half and y is a half tensor; y and its guard bands then
    start as the finite Y16_CANARY, and no element of y may still hold it after a launch."""
    L = _lib.lib()
    B, c0, H, W = x.shape
    dev = x.device
    cout, k = w.shape[0], w.shape[-1]
    w, b, x = _lib.f32c(w), _lib.f32c(b), _io(x, io16)
    if x1 is not None:
        x1 = _io(x1, io16)
    cin = w.shape[1]
    if c1 is None:
        c1 = 0 if x1 is None else x1.shape[1]
        assert c0 + c1 == cin
    if residual is not None:
        residual = residual.detach().half().contiguous() if io16 & 2 else _lib.f32c(residual)
        assert residual.shape == ((cout, H, W) if res_broadcast else (B, cout, H, W))
    packed = torch.full((L.r2dm_conv_packed_elems(cout, cin, k, B, H, W),), float("nan"), device=dev)  # (a refusal comes before the weights are packed)
    yg = (H * W + 63) // 64 * 64  # one plane, in whole 256-byte lines (the kernels store 16-byte vectors)
    fill = Y16_CANARY if io16 & 2 else float("nan")
    y_all, y = guarded((B, cout, H, W), torch.float16 if io16 & 2 else torch.float32, yg, dev, fill=fill)
    st_all = stat = None
    if stat_groups:
        st_all, stat = guarded((B, stat_groups, L.r2dm_conv_stat_slots(H, W), 2), torch.float64, 64, dev)
    rng = None if range_init is None else torch.tensor(list(range_init), device=dev, dtype=torch.int32)
    sc = None if scale is None else torch.tensor([scale], device=dev, dtype=torch.float32)
    chosen = (ctypes.c_int32 * 3)(-1, -1, -1)
    rc = L.r2dm_conv2d_ring_ex(x.data_ptr(), _lib.ptr(x1), c1, w.data_ptr(), b.data_ptr(), packed.data_ptr(), _lib.ptr(aff), prologue, _lib.ptr(residual),
                               int(res_broadcast), _lib.ptr(sc), y.data_ptr(), _lib.ptr(stat), stat_groups, stat_goff, stat_cpg, _lib.ptr(rng), reverse,
                               ctypes.addressof(chosen), B, cin, cout, H, W, k, _st(x))
    torch.cuda.synchronize()
    if rc != 0:
        assert fill_intact(y_all, fill) and (st_all is None or torch.isnan(st_all).all()), "a refused launch wrote to y or to the sink"
        assert rng is None or rng.tolist() == list(range_init), "a refused launch wrote to the range record"
        assert torch.isnan(packed).all(), "a refused launch wrote to the packed weights"
        _lib.check(rc)
    assert guard_intact(y_all, yg, fill), "write outside y"
    assert not io16 & 2 or not bool((y == Y16_CANARY).any()), "an output element was not written"
    assert st_all is None or guard_intact(st_all, 64), "write outside the statistics sink"
    return ConvExResult(y, stat, None if rng is None else rng.cpu(), tuple(chosen))


def group_norm_affine(x, groups, eps, gamma=None, beta=None, ada=None):
    L = _lib.lib()
    B, C, H, W = x.shape
    x = _lib.f32c(x)
    scratch = torch.empty(L.r2dm_group_norm_scratch_bytes(B, groups), dtype=torch.uint8, device=x.device)
    aff = torch.empty(B, C, 2, device=x.device)
    stats = torch.empty(B, groups, 2, device=x.device)
    _lib.check(L.r2dm_group_norm_affine(x.data_ptr(), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ada), scratch.data_ptr(),
                                        aff.data_ptr(), stats.data_ptr(), B, C, H, W, groups, eps, _st(x)))
    torch.cuda.synchronize()
    return aff, stats


def group_norm_from_stats(stat, C, H, W, eps, gamma=None, beta=None, ada=None):
    """(aff, stats) of gn_finalize_kernel over a statistics sink (B, groups, slots, 2) float64 as a producer's epilogue left it."""
    B, groups, slots, two = stat.shape
    assert two == 2 and stat.dtype == torch.float64 and stat.is_contiguous()
    aff = torch.empty(B, C, 2, device=stat.device)
    stats = torch.empty(B, groups, 2, device=stat.device)
    _lib.check(_lib.lib().r2dm_group_norm_from_stats(stat.data_ptr(), slots, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ada), aff.data_ptr(), stats.data_ptr(),
                                                     B, C, H, W, groups, eps, _st(stat)))
    torch.cuda.synchronize()
    return aff, stats


# ---- the range guard's other producers: the _ex entries with a record ------------------------------------------------------------------------
RANGE_FLAG = 7  # what [0] of a record holds around a call: the producers never write it


def float_bits(v):
    """The int32 bit pattern of float32(v)."""
    return int(torch.tensor([v], dtype=torch.float32).view(torch.int32).item())


def bits_float(b):
    """float32 of an int32 bit pattern, as a Python float."""
    return float(torch.tensor([b], dtype=torch.int32).view(torch.float32).item())


def _record(range_init, dev):
    """The device int32[2] a call starts from: (RANGE_FLAG, bits of range_init); None: no record."""
    return None if range_init is None else torch.tensor([RANGE_FLAG, float_bits(range_init)], device=dev, dtype=torch.int32)


def _recorded(rng):
    """The record after the call: the bits of [1] (None without a record); [0] must be untouched."""
    if rng is None:
        return None
    flag, bits = rng.cpu().tolist()
    assert flag == RANGE_FLAG, f"the producer wrote {flag} to [0] of the range record"
    return bits


def group_norm_affine_ex(x, groups, eps, gamma=None, beta=None, ada=None, range_init=None):
    """(aff, stats, record bits): r2dm_group_norm_affine_ex -- the streaming pass, M = the recorded max|x|.  aff and stats start NaN-filled inside NaN
    guard bands that must survive the call; range_init: the float the record starts from (None: no record)."""
    L = _lib.lib()
    B, C, H, W = x.shape
    x = _lib.f32c(x)
    scratch = torch.empty(L.r2dm_group_norm_scratch_bytes(B, groups), dtype=torch.uint8, device=x.device)
    aff_all, aff = guarded((B, C, 2), torch.float32, 64, x.device)
    st_all, stats = guarded((B, groups, 2), torch.float32, 64, x.device)
    rng = _record(range_init, x.device)
    _lib.check(L.r2dm_group_norm_affine_ex(x.data_ptr(), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ada), scratch.data_ptr(), aff.data_ptr(), stats.data_ptr(),
                                           B, C, H, W, groups, eps, _st(x), _lib.ptr(rng)))
    torch.cuda.synchronize()
    assert guard_intact(aff_all, 64) and guard_intact(st_all, 64), "write outside aff / stats"
    return aff, stats, _recorded(rng)


def group_norm_from_stats_ex(stat, C, H, W, eps, gamma=None, beta=None, ada=None, range_init=None):
    """(aff, stats, record bits): r2dm_group_norm_from_stats_ex over a sink (B, groups, slots, 2) float64 -- M = sqrt(largest slot energy); outputs
    and record as group_norm_affine_ex."""
    B, groups, slots, two = stat.shape
    assert two == 2 and stat.dtype == torch.float64 and stat.is_contiguous()
    aff_all, aff = guarded((B, C, 2), torch.float32, 64, stat.device)
    st_all, stats = guarded((B, groups, 2), torch.float32, 64, stat.device)
    rng = _record(range_init, stat.device)
    _lib.check(_lib.lib().r2dm_group_norm_from_stats_ex(stat.data_ptr(), slots, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ada), aff.data_ptr(), stats.data_ptr(),
                                                        B, C, H, W, groups, eps, _st(stat), _lib.ptr(rng)))
    torch.cuda.synchronize()
    assert guard_intact(aff_all, 64) and guard_intact(st_all, 64), "write outside aff / stats"
    return aff, stats, _recorded(rng)


def fir_up2_ex(x, io16=0, range_init=None):
    """(y, record bits): r2dm_fir_up2_ex; io16 as fir_up2 (with R2DM_TEST_IO16 set by the caller).  y starts NaN-filled inside NaN guard bands of one
    output row pair that must survive the call, and every element of it must have been written (a finite input leaves no NaN)."""
    B, C, H, W = x.shape
    x = _io(x, io16)
    yg = (4 * W + 63) // 64 * 64
    y_all, y = guarded((B, C, H * 2, W * 2), torch.float16 if io16 & 2 else torch.float32, yg, x.device)
    rng = _record(range_init, x.device)
    _lib.check(_lib.lib().r2dm_fir_up2_ex(x.data_ptr(), y.data_ptr(), B, C, H, W, _st(x), _lib.ptr(rng)))
    torch.cuda.synchronize()
    assert guard_intact(y_all, yg), "write outside y"
    return y, _recorded(rng)


def down_planes_ex(x, range_init=None):
    """(planes (B, 9 C, H / 2, W / 2), record bits): r2dm_down_planes_ex; the planes start NaN-filled inside NaN guard bands of one plane."""
    B, C, H, W = x.shape
    x = _lib.f32c(x)
    g = ((H // 2) * (W // 2) + 63) // 64 * 64
    a_all, a = guarded((B, 9 * C, H // 2, W // 2), torch.float32, g, x.device)
    rng = _record(range_init, x.device)
    _lib.check(_lib.lib().r2dm_down_planes_ex(x.data_ptr(), a.data_ptr(), B, C, H, W, _st(x), _lib.ptr(rng)))
    torch.cuda.synchronize()
    assert guard_intact(a_all, g), "write outside the planes"
    return a, _recorded(rng)


def down_phase_planes_ex(x, range_init=None):
    """(planes (B, 2, C, H + 3, W / 2 + 4), record bits): r2dm_down_phase_planes_ex; the buffer starts NaN-filled inside NaN guard bands of one
    channel's rows -- what is still NaN after the call, the kernel did not write (floats 0 .. 2 of every row, float 3 of the second phase's)."""
    L = _lib.lib()
    B, C, H, W = x.shape
    x = _lib.f32c(x)
    assert L.r2dm_down_phase_planes_floats(C, H, W) == 2 * C * (H + 3) * (W // 2 + 4)
    g = ((H + 3) * (W // 2 + 4) + 63) // 64 * 64
    a_all, a = guarded((B, 2, C, H + 3, W // 2 + 4), torch.float32, g, x.device)
    rng = _record(range_init, x.device)
    _lib.check(L.r2dm_down_phase_planes_ex(x.data_ptr(), a.data_ptr(), B, C, H, W, _st(x), _lib.ptr(rng)))
    torch.cuda.synchronize()
    assert guard_intact(a_all, g), "write outside the phase planes"
    return a, _recorded(rng)


def affine_act(x, aff, silu):
    L = _lib.lib()
    B, C, H, W = x.shape
    y = torch.empty_like(x)
    _lib.check(L.r2dm_affine_act(x.data_ptr(), aff.data_ptr(), y.data_ptr(), B, C, H * W, int(silu), _st(x)))
    torch.cuda.synchronize()
    return y


def _io(x, io16):
    return x.detach().half().contiguous() if io16 & 1 else _lib.f32c(x)


def fir_down2(x, io16=0):
    """io16 (with R2DM_TEST_IO16 set to the same value by the caller): bit 0 -- x as a half tensor, bit 1 -- y will be one."""
    B, C, H, W = x.shape
    x = _io(x, io16)
    y = torch.empty(B, C, H // 2, W // 2, device=x.device, dtype=torch.float16 if io16 & 2 else torch.float32)
    _lib.check(_lib.lib().r2dm_fir_down2(x.data_ptr(), y.data_ptr(), B, C, H, W, _st(x)))
    torch.cuda.synchronize()
    return y


def fir_down2_stats(x, groups, io16=0):
    """(y, stat): ops.Resample(down=2) plus the GroupNorm statistics of y as the engine's path leaves them -- stat (B, groups, slots, 2)
    float64 [sum, sum of squares]; None where the geometry has no statistics variant."""
    B, C, H, W = x.shape
    slots = _lib.lib().r2dm_fir_down2_stat_slots(C, groups, H, W)
    if slots == 0:
        return None
    x = _io(x, io16)
    y = torch.empty(B, C, H // 2, W // 2, device=x.device, dtype=torch.float16 if io16 & 2 else torch.float32)
    stat = torch.full((B, groups, slots, 2), float("nan"), device=x.device, dtype=torch.float64)
    _lib.check(_lib.lib().r2dm_fir_down2_stats(x.data_ptr(), y.data_ptr(), stat.data_ptr(), B, C, groups, H, W, _st(x)))
    torch.cuda.synchronize()
    return y, stat


def down_planes(x):
    """resample.hip's down_planes_kernel: the nine FIR planes of every channel, (B, 9 C, H / 2, W / 2)."""
    B, C, H, W = x.shape
    x = _lib.f32c(x)
    a = torch.full((B, 9 * C, H // 2, W // 2), float("nan"), device=x.device)
    _lib.check(_lib.lib().r2dm_down_planes(x.data_ptr(), a.data_ptr(), B, C, H, W, _st(x)))
    torch.cuda.synchronize()
    return a


def down_gemm(x, w, b, groups=0, nine=False):
    """(y, stat): Resample(down=2)(Conv3x3(x)) through the pre-pass and the GEMM -- r2dm_down_gemm (every distinct plane stored once), or, `nine`,
    r2dm_down_gemm_nine (all nine planes); stat (B, groups, slots, 2) float64 or None.  y starts NaN-filled between NaN guard bands of one plane that must
    survive the call."""
    L = _lib.lib()
    B, cin, H, W = x.shape
    cout = w.shape[0]
    x, w, b = _lib.f32c(x), _lib.f32c(w), _lib.f32c(b)
    packed = torch.empty(9 * cin * cout + 64, device=x.device)
    planes = torch.empty(B * 9 * cin * (H // 2) * (W // 2), device=x.device)
    yg = ((H // 2) * (W // 2) + 63) // 64 * 64
    y_all, y = guarded((B, cout, H // 2, W // 2), torch.float32, yg, x.device)
    stat = None
    if groups:
        slots = L.r2dm_down_gemm_stat_slots(cin, cout, groups, H, W)
        assert slots > 0
        stat = torch.full((B, groups, slots, 2), float("nan"), device=x.device, dtype=torch.float64)
    entry = L.r2dm_down_gemm_nine if nine else L.r2dm_down_gemm
    _lib.check(entry(x.data_ptr(), w.data_ptr(), b.data_ptr(), packed.data_ptr(), planes.data_ptr(), y.data_ptr(), _lib.ptr(stat),
                     B, cin, cout, groups, H, W, _st(x)))
    torch.cuda.synchronize()
    assert guard_intact(y_all, yg), "write outside y"
    return y, stat


def fir_up2(x, io16=0):
    B, C, H, W = x.shape
    x = _io(x, io16)
    y = torch.empty(B, C, H * 2, W * 2, device=x.device, dtype=torch.float16 if io16 & 2 else torch.float32)
    _lib.check(_lib.lib().r2dm_fir_up2(x.data_ptr(), y.data_ptr(), B, C, H, W, _st(x)))
    torch.cuda.synchronize()
    return y


def attention(qkv, heads):
    B, C3, N = qkv.shape
    C = C3 // 3
    out = torch.empty(B, C, N, device=qkv.device)
    _lib.check(_lib.lib().r2dm_attention(qkv.data_ptr(), out.data_ptr(), B, C, heads, N, _st(qkv)))
    torch.cuda.synchronize()
    return out


_CANARY = 0x7FC5A5A5  # a quiet NaN with a payload: no arithmetic produces these bits


def attention_padded(qkv, heads, C=None):
    """r2dm_attention into the middle of a canary-filled buffer of (C + 2) N floats: the N-float row before the output and the one after it must
    come back bit-unchanged (rows of at least 64 floats, so that N = 0 is still guarded).  If the entry refuses, the whole buffer must be, and the
    error is raised on.  C overrides the channel count (for the refusal tests)."""
    B, C3, N = qkv.shape
    C = C3 // 3 if C is None else C
    row = max(N, 64)
    whole, out = guarded((B, C, N), torch.int32, row, qkv.device, fill=_CANARY)
    out = out.view(torch.float32)
    rc = _lib.lib().r2dm_attention(qkv.data_ptr(), out.data_ptr(), B, C, heads, N, _st(qkv))
    torch.cuda.synchronize()
    if rc != 0:
        assert bool((whole == _CANARY).all()), "a refused launch wrote to the output"
        _lib.check(rc)
    assert bool((whole[:row] == _CANARY).all() and (whole[-row:] == _CANARY).all()), "write outside the output"
    assert not bool((out.view(torch.int32) == _CANARY).any()), "an output element was not written"
    return out


def in_guard(t, guard=64, offset=0):
    """A float32 copy of t as a contiguous view, `guard + offset` floats into a NaN-filled allocation that goes on `guard` floats past its end: a
    read past either end of it turns the result NaN instead of faulting.  (guard = 64: 256 bytes, the view keeps the allocation's alignment.)"""
    t = _lib.f32c(t)
    whole = torch.full((guard + offset + t.numel() + guard,), float("nan"), device=t.device)
    view = whole[guard + offset:guard + offset + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def time_embedding(cond, freqs, w1, b1, w2, b2, return_hidden=False):
    """act (B, T) = SiLU(time_embedding(cond)) -- with return_hidden (act, hidden), hidden (B, T) = SiLU of the first Linear.  Both start NaN-filled
    inside NaN guard bands that must survive the call, and with finite operands every element of them must have been written; the operands are views
    into NaN-filled allocations (in_guard)."""
    B, T, base = cond.shape[0], w1.shape[0], w1.shape[1]
    ops = [in_guard(t) for t in (cond, freqs, w1, b1, w2, b2)]
    act_all, act = guarded((B, T), torch.float32, 64, cond.device)
    hid_all, hid = guarded((B, T), torch.float32, 64, cond.device)
    _lib.check(_lib.lib().r2dm_time_embedding(*(t.data_ptr() for t in ops), act.data_ptr(), hid.data_ptr(), B, base, T, _st(cond)))
    torch.cuda.synchronize()
    assert guard_intact(act_all, 64) and guard_intact(hid_all, 64), "write outside act / hidden"
    if all(bool(torch.isfinite(t).all()) for t in ops):
        assert not bool(torch.isnan(act).any() or torch.isnan(hid).any()), "an element of act / hidden was not written, or a read left an operand"
    return (act, hid) if return_hidden else act


def ada_proj(act, w, bias, w_offset=0):
    """out (B, rows) = r2dm_ada_proj(act (B, T), w (rows, T), bias (rows,)).  out starts NaN-filled inside NaN guard bands that must survive the call;
    act and w are views into NaN-filled allocations (in_guard; w_offset: floats to shift w by, for the alignment refusal), so with finite operands a
    NaN in out is an element that was not written or a read past an operand's end.  If the entry refuses, out must still be NaN throughout, and the
    error is raised on."""
    (B, T), rows = act.shape, w.shape[0]
    assert w.shape == (rows, T) and bias.shape == (rows,)
    act, w, bias = in_guard(act), in_guard(w, offset=w_offset), _lib.f32c(bias)
    out_all, out = guarded((B, rows), torch.float32, 64, act.device)
    rc = _lib.lib().r2dm_ada_proj(act.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B, T, rows, _st(act))
    torch.cuda.synchronize()
    if rc != 0:
        assert bool(torch.isnan(out_all).all()), "a refused launch wrote to out"
        _lib.check(rc)
    assert guard_intact(out_all, 64), "write outside out"
    if all(bool(torch.isfinite(t).all()) for t in (act, w, bias)):
        assert not bool(torch.isnan(out).any()), "an element of out was not written, or a read left act / w"
    return out


def group_norm_from_stats_strided(stat, C, H, W, eps, ada, ada_stride, gamma=None, beta=None, range_init=None):
    """(aff, stats, record bits): r2dm_group_norm_from_stats_strided -- group_norm_from_stats_ex with sample b's AdaGN row [scale(C) | shift(C)] at
    ada + b ada_stride floats (ada: a tensor whose first element is sample 0's scale; the caller owns what lies around it); outputs and record as
    group_norm_from_stats_ex.  If the entry refuses, aff and stats must still be NaN throughout, and the error is raised on."""
    B, groups, slots, two = stat.shape
    assert two == 2 and stat.dtype == torch.float64 and stat.is_contiguous()
    aff_all, aff = guarded((B, C, 2), torch.float32, 64, stat.device)
    st_all, stats = guarded((B, groups, 2), torch.float32, 64, stat.device)
    rng = _record(range_init, stat.device)
    rc = _lib.lib().r2dm_group_norm_from_stats_strided(stat.data_ptr(), slots, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(ada), ada_stride, aff.data_ptr(),
                                                       stats.data_ptr(), B, C, H, W, groups, eps, _st(stat), _lib.ptr(rng))
    torch.cuda.synchronize()
    if rc != 0:
        assert bool(torch.isnan(aff_all).all() and torch.isnan(st_all).all()), "a refused launch wrote to aff / stats"
        _lib.check(rc)
    assert guard_intact(aff_all, 64) and guard_intact(st_all, 64), "write outside aff / stats"
    return aff, stats, _recorded(rng)
