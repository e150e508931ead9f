"""What the CPU preconditions (test_proj_cases_cpu.py) and the GPU tests (test_hip_proj.py) of proj_f16x2.hip share: the table of the kernel's 13
instantiations with the entry that reaches each, the shape rows, the input generators, the fp64 references and a Python mirror of the dispatch rule
(launch_proj_f16x2).  Numpy / torch on the CPU, integer seeds, no GPU.

The kernel:  Y[b][co][px] = sum_ci W[co][ci] f(X[b][ci][px]) + bias (+ residual) (* scale), f = identity (PRO_NONE) or x a[b][ci] + d[b][ci] (PRO_AFFINE);
operands split v = h + 2^-11 l (f16x2.h), weights scaled by the power of two that brings max|w| into [2^9, 2^10), products h h into one fp32 accumulator,
h l + l h into a second one (NPLK = 2) or h h alone (NPLK = 1).  The down-sampling GEMMs are the same product over the nine FIR planes of a 3x3 convolution's
input (K = 9 Cin), with the bias scaled by the FIR's row factor (FIRB), the planes stored nine times (r2dm_down_gemm_nine) or once per phase (PHP).

Exact-grid inputs (a).  Products, every partial sum of either accumulator in any order, and the epilogue are exactly representable, so the kernel must
return the fp64 result rounded to fp32 (Y16: rounded once more to fp16) whatever its summation order:
  * the x operand of the product (after the affine, after the FIR) is a multiple of 2^-12 with |v| <= 3: h is a multiple of 2^-12, l = 2^11 (v - h) a multiple of
    1/2 with |l| <= 2, neither an fp16 subnormal; one-plane rows use values that are fp16 numbers themselves (2^-9 grid, |v| < 4), so that h = v.
  * weights in {-2 .. 2} with +-2 in every 64-channel slice: scale 2^8, wh a multiple of 256 with |wh| <= 512, wl = 0.
  * every product is then a multiple of g = 2^-4 (h h) or 2^7 (l h), and sum_k |product| <= K 3 512 < 2^24 g for K <= 576: every partial sum in every order
    is a multiple of g below 2^24 g, i.e. an fp32 number.  test_proj_cases_cpu.py asserts the grids and this sum bound on the data, and repeats the kernel's
    arithmetic in fp32 in a random order.
  * epilogue: acc + 2^-11 acl and the 2^-8 of the weight scale are exact; bias and residual are multiples of 2^-12 in [-1, 1), the scale is 1/2.
  * with wl = 0 this grid cannot see the weights' l plane; exact_inputs_split_weights is its counterpart for that plane (twelve-bit weights, a coarse x).
Benign inputs (b, c): N(0, 1) data, weights / sqrt(K) -- with the layer's max|w| planted (random sign) in every 64-channel slice, so that a launch on a
slice has the whole layer's weight scale --, residual and 1/sqrt(2) where the instantiation takes them."""
import math
import os
import re
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "r2dm_amd", "csrc", "proj_f16x2.hip")

PRO_NONE, PRO_AFFINE = 0, 1
Inst = namedtuple("Inst", "tall pro nplk iom firb php")  # proj_f16x2_kernel<TALL, PRO, NPLK, IOM, FIRB, PHP>

# the issue's table: instantiation -> the single-kernel entry that reaches it ("ring": r2dm_conv2d_ring[_ex] with k = 1; pieces = NPLK through
# r2dm_set_conv_pieces; IOM 3: R2DM_TEST_IO16 = 3)
TABLE = {}
for _tall in (0, 1):
    for _pro in (PRO_NONE, PRO_AFFINE):
        for _nplk in (2, 1):
            TABLE[Inst(_tall, _pro, _nplk, 0, 0, 0)] = "ring"
    TABLE[Inst(_tall, PRO_NONE, 2, 0, 1, 0)] = "nine"   # r2dm_down_gemm_nine
    TABLE[Inst(_tall, PRO_NONE, 2, 0, 1, 1)] = "phase"  # r2dm_down_gemm
TABLE[Inst(0, PRO_NONE, 1, 3, 0, 0)] = "ring"            # pieces 1 and R2DM_TEST_IO16 = 3: wide even where Cout % 256 == 0
assert len(TABLE) == 13

CKP, CO_T, COB, TH, TW = 32, 64, 256, 4, 64  # namespace p1


def supported(K, cout, h, w):
    """proj_f16x2_supported (taps = 1)."""
    return K % CKP == 0 and cout % CO_T == 0 and h % TH == 0 and w % TW == 0


def dispatch(K, cout, h, w, pieces=2, prologue=0, io16=0, down=None, residual=False, stat=False, seam=None):
    """launch_proj_f16x2, line by line: the instantiation a launch runs, or None where the launcher refuses.  K, h, w: the GEMM's depth and pixel grid
    (down: 9 Cin and the OUTPUT size); down: None | "nine" | "phase"; seam: channels in the first of two allocations, None for one source."""
    if not supported(K, cout, h, w) or (seam is not None and seam % 8) or prologue not in (PRO_NONE, PRO_AFFINE):
        return None
    x16, y16 = io16 & 1, (io16 >> 1) & 1
    if x16 or y16:
        if not (x16 and y16) or pieces != 1 or prologue != PRO_NONE or residual or stat:
            return None
        return Inst(0, PRO_NONE, 1, 3, 0, 0)
    tall = int(cout % COB == 0)
    if down is not None:
        if pieces == 1 or prologue != PRO_NONE or residual:
            return None
        if down == "phase":
            return None if seam is not None or K % (9 * CKP) else Inst(tall, PRO_NONE, 2, 0, 1, 1)
        return Inst(tall, PRO_NONE, 2, 0, 1, 0)
    return Inst(tall, prologue, 1 if pieces == 1 else 2, 0, 0, 0)


def source_instantiations():
    """Every launch_p1<...> inside launch_proj_f16x2 (proj_f16x2.hip), as Inst tuples with the template's defaults filled in."""
    text = open(SOURCE).read()
    body = text[text.index("hipError_t launch_proj_f16x2("):]
    body = body[:body.index("\n}\n")]  # (the function's closing brace: the first one in column 0)
    val = {"true": 1, "false": 0, "PRO_NONE": PRO_NONE, "PRO_AFFINE": PRO_AFFINE}
    found = set()
    for m in re.finditer(r"launch_p1<([^>]*)>\s*\(", body):
        args = [val[a] if a in val else int(a) for a in (s.strip() for s in m.group(1).split(","))]
        found.add(Inst(*(args + [0, 0, 0][len(args) - 3:])))
    return found


# ---- shapes: the smallest at which each index can still go wrong ---------------------------------------------------------------------------
# Case.cin / h / w: the convolution's input channels and INPUT size (down: the GEMM runs at K = 9 cin on h / 2 x w / 2)
Case = namedtuple("Case", "inst entry cin cout h w B")
WIDE_1X1 = [(32, 64, 4, 64, 1),      # one chunk, one block
            (96, 128, 8, 128, 2)]    # three chunks (the pipeline's steady state, an odd count), two channel blocks, 2 x 2 pixel tiles
TALL_1X1 = [(32, 256, 4, 64, 1),
            (96, 512, 8, 128, 3)]    # nCoB = 2: cob runs fastest, then the tile row
IOM_SHAPES = [(96, 128, 8, 128, 2),
              (32, 256, 4, 64, 2)]   # Cout % 256 == 0 and still the wide kernel
DOWN_SHAPES = [(32, 64, 8, 128, 3),
               (64, 128, 16, 256, 1),   # 2 x 2 output tiles
               (32, 256, 8, 128, 2),
               (32, 512, 16, 128, 1)]   # tall, nCoB = 2, two tile rows: down_phase_row's border and interior rows


def _cases():
    out = []
    for shapes in (WIDE_1X1, TALL_1X1):
        for s in shapes:
            for pro in (PRO_NONE, PRO_AFFINE):
                for nplk in (2, 1):
                    out.append(Case(Inst(int(s[1] % COB == 0), pro, nplk, 0, 0, 0), "ring", *s))
    for s in IOM_SHAPES:
        out.append(Case(Inst(0, PRO_NONE, 1, 3, 0, 0), "ring", *s))
    for s in DOWN_SHAPES:
        for entry in ("nine", "phase"):
            out.append(Case(Inst(int(s[1] % COB == 0), PRO_NONE, 2, 0, 1, int(entry == "phase")), entry, *s))
    return out


CASES = _cases()
TALL_CASES = [c for c in CASES if c.inst.tall]


def inst_id(i):
    return (("tall" if i.tall else "wide") + ("-affine" if i.pro else "") + f"-p{i.nplk}" + ("-io16" if i.iom else "")
            + ("-phase" if i.php else "-nine" if i.firb else ""))


def case_id(c):
    return f"{inst_id(c.inst)}-{c.cin}-{c.cout}-{c.h}x{c.w}-B{c.B}"


def is_down(c):
    return c.entry != "ring"


def gemm_shape(c):
    """(K, h, w) of the launch itself."""
    return (9 * c.cin, c.h // 2, c.w // 2) if is_down(c) else (c.cin, c.h, c.w)


def launch_args(c):
    """What dispatch() is asked for the case."""
    K, h, w = gemm_shape(c)
    return dict(K=K, cout=c.cout, h=h, w=w, pieces=c.inst.nplk, prologue=c.inst.pro, io16=c.inst.iom, down=c.entry if is_down(c) else None,
                residual=takes_residual(c))


def takes_residual(c):
    """Residual and scale: the 1x1 launches with fp32 storage (the down-sampling GEMM and the fp16-storage launch take neither)."""
    return c.entry == "ring" and c.inst.iom == 0


# ---- generators ----------------------------------------------------------------------------------------------------------------------------
SCALE_EXACT = 0.5
SCALE_BENIGN = float(np.float32(0.70710678))  # the value the kernel reads


def _gen(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _grid(g, step, lo, hi, shape):
    """Integer multiples of `step` in [lo, hi], float32 (exact)."""
    return torch.from_numpy((g.integers(round(lo / step), round(hi / step), shape, endpoint=True) * step).astype(np.float32))


def _seed(c, base):
    return base + 7 * c.cin + 3 * c.cout + c.h + c.w + 11 * c.B + 13 * c.inst.pro + 17 * c.inst.nplk + 19 * c.inst.iom


def weight_shape(c):
    return (c.cout, c.cin, 3, 3) if is_down(c) else (c.cout, c.cin, 1, 1)


def plant(w, g, value):
    """+-value at one random place of every 64-channel slice of w (in place): every slice then has the layer's max|w|, hence its weight scale."""
    per = w[0].numel()
    for s in range(w.shape[0] // CO_T):
        i = int(g.integers(0, CO_T * per))
        w[s * CO_T + i // per].view(-1)[i % per] = value * (1.0 if g.integers(0, 2) else -1.0)
    return w


def exact_inputs(c, seed=1000):
    """dict(x, w, b, res, scale, aff) on the grids of the module docstring."""
    g = _gen(_seed(c, seed))
    two = c.inst.nplk == 2
    if is_down(c):  # 2^-6 at the input (the 16-tap FIR's coefficients are multiples of 2^-6: planes on 2^-12); a per-channel level of 1/2 .. 7/8 under the noise,
        # so that the smoothed planes keep magnitudes in [1/2, 1), where 2^-12 lies below fp16's spacing and the l plane is in use
        level = _grid(g, 2.0 ** -6, 0.5, 0.875, (c.B, c.cin, 1, 1)) * torch.from_numpy(g.choice([-1.0, 1.0], (c.B, c.cin, 1, 1)).astype(np.float32))
        x = level + _grid(g, 2.0 ** -6, -0.125, 0.125, (c.B, c.cin, c.h, c.w))
    elif c.inst.pro:
        x = _grid(g, 2.0 ** (-11 if two else -8), -1, 1, (c.B, c.cin, c.h, c.w))
    else:
        x = _grid(g, 2.0 ** (-12 if two else -9), -1, 1, (c.B, c.cin, c.h, c.w))
    w = plant(_grid(g, 1.0, -2, 2, weight_shape(c)), g, 2.0)
    b = _grid(g, 2.0 ** -12, -1, 1 - 2.0 ** -12, (c.cout,))
    res = _grid(g, 2.0 ** -12, -1, 1 - 2.0 ** -12, (c.B, c.cout, c.h, c.w)) if takes_residual(c) else None
    aff = None
    if c.inst.pro:
        a = torch.from_numpy(g.choice([0.5, 1.0, 2.0], (c.B, c.cin)).astype(np.float32))
        aff = torch.stack([a, _grid(g, 2.0 ** (-12 if two else -9), -1, 1 - 2.0 ** -9, (c.B, c.cin))], -1).contiguous()
    return dict(x=x, w=w, b=b, res=res, scale=SCALE_EXACT if res is not None else None, aff=aff)


SPLIT_WEIGHT_CASES = [c for c in CASES if c.entry == "ring" and c.inst.nplk == 2]


def exact_inputs_split_weights(c, seed=3000):
    """The exact grid above has wl = 0: it cannot see the weights' l plane.  Its counterpart for that plane, for the two-plane 1x1 rows: weights n / 4096 with
    |n| <= 4095 and +-4095 in every 64-channel slice -- scale 2^10, w s = n / 4 with twelve bits, wh a multiple of 1/4 up to 1024 and wl = 2^11 (w s - wh) in
    {0, +-512} wherever |w s| >= 512 has an odd quarter -- against a COARSE x operand, a multiple of 1/4 with |v| <= 3 (x on 1/4, or on 1/2 with a in {1/2, 1, 2} and
    d on 1/4), whose own l plane is zero.  Products: wh xh multiples of 2^-4 and wl xh multiples of 2^7, sum_k |product| <= 96 . 3 . 1024 = 2^18.2 < 2^24 . 2^-4; the
    epilogue's 2^-10 leaves multiples of 2^-14 below 2^9: 23 bits, bias and residual (2^-12) included."""
    assert c.entry == "ring" and c.inst.nplk == 2 and c.cin <= 96
    g = _gen(_seed(c, seed))
    x = _grid(g, 0.5 if c.inst.pro else 0.25, -1, 1, (c.B, c.cin, c.h, c.w))
    w = plant(_grid(g, 1.0 / 4096, -4095.0 / 4096, 4095.0 / 4096, weight_shape(c)), g, 4095.0 / 4096)
    b = _grid(g, 2.0 ** -12, -1, 1 - 2.0 ** -12, (c.cout,))
    res = _grid(g, 2.0 ** -12, -1, 1 - 2.0 ** -12, (c.B, c.cout, c.h, c.w))
    aff = None
    if c.inst.pro:
        a = torch.from_numpy(g.choice([0.5, 1.0, 2.0], (c.B, c.cin)).astype(np.float32))
        aff = torch.stack([a, _grid(g, 0.25, -1, 0.75, (c.B, c.cin))], -1).contiguous()
    return dict(x=x, w=w, b=b, res=res, scale=SCALE_EXACT, aff=aff)


def benign_inputs(c, seed=2000):
    """dict(x, w, b, res, scale, aff): N(0, 1) data.  One-plane rows with the affine: x on the 2^-9 grid, a in {1/2, 1, 2}, d on 2^-12 -- x a + d is then
    exact in fp32 with or without FMA contraction (a multiple of 2^-12 below 16: 16 bits), and its ONE rounding to fp16 is what the emulation takes.
    Two-plane rows: (a, d) = (U(0.5, 1.5), 0.3 N(0, 1)), test_conv1x1_fp16_pipe_and_fp32_mfma's.  The fp16-storage row: x rounded to fp16."""
    g = _gen(_seed(c, seed))
    n = lambda *shape: torch.from_numpy(g.standard_normal(shape).astype(np.float32))
    x = n(c.B, c.cin, c.h, c.w)
    aff = None
    if c.inst.pro and c.inst.nplk == 1:
        x = torch.round(x * 512) / 512
        a = torch.from_numpy(g.choice([0.5, 1.0, 2.0], (c.B, c.cin)).astype(np.float32))
        aff = torch.stack([a, _grid(g, 2.0 ** -12, -1, 1 - 2.0 ** -12, (c.B, c.cin))], -1).contiguous()
    elif c.inst.pro:
        aff = torch.stack([torch.from_numpy(g.random((c.B, c.cin)).astype(np.float32)) + 0.5, n(c.B, c.cin) * 0.3], -1).contiguous()
    if c.inst.iom & 1:
        x = x.half().float()
    w = n(*weight_shape(c)) / math.sqrt(gemm_shape(c)[0])
    w = plant(w, g, w.abs().max().item())
    res = n(c.B, c.cout, c.h, c.w) if takes_residual(c) else None
    return dict(x=x, w=w, b=n(c.cout), res=res, scale=SCALE_BENIGN if res is not None else None, aff=aff)


# ---- references ----------------------------------------------------------------------------------------------------------------------------
FIR = (0.125, 0.375, 0.375, 0.125)


def down_planes(x):
    """The nine FIR planes of resample.hip's down_planes_kernel in x's dtype, (B, 9 C, H / 2, W / 2), plane (ky 3 + kx) C + c:
        V[ky][i][c]     = sum_t f[t] [0 <= 2i-1+t < H] x[2i-1+t + ky-1][c]         f = [1,3,3,1]/8, x zero outside rows [0, H)
        A[ky][kx][i][j] = sum_t f[t] V[ky][i][(2j + t + kx - 2) mod W]"""
    B, C, H, W = x.shape
    xz = x.new_zeros(B, C, H + 6, W)  # row r of x at xz[r + 3]
    xz[:, :, 3:H + 3] = x
    i2, cols = torch.arange(H // 2) * 2, torch.arange(W // 2) * 2
    A = x.new_zeros(B, 3, 3, C, H // 2, W // 2)
    for ky in range(3):
        V = x.new_zeros(B, C, H // 2, W)
        for t in range(4):
            r = i2 - 1 + t
            V += FIR[t] * ((r >= 0) & (r < H)).to(x.dtype)[:, None] * xz[:, :, r + ky + 2]
        for kx in range(3):
            for t in range(4):
                A[:, ky, kx] += FIR[t] * V[..., (cols + t + kx - 2) % W]
    return A.reshape(B, 9 * C, H // 2, W // 2)


def weight_matrix(c, w):
    """(Cout, K): the packer's column order -- (ky 3 + kx) Cin + ci for the down-sampling GEMM."""
    return w.permute(0, 2, 3, 1).reshape(c.cout, -1) if is_down(c) else w.reshape(c.cout, -1)


def x_operand(c, d, dtype):
    """The product's x operand evaluated in `dtype`: after the affine, after the FIR; (B, K, h, w)."""
    x = d["x"].to(dtype)
    if d["aff"] is not None:
        a = d["aff"].to(dtype)
        x = x * a[..., 0, None, None] + a[..., 1, None, None]
    return down_planes(x) if is_down(c) else x


def row_factor(c, dtype=torch.float64):
    """FIRB: the bias went through the zero-padded FIR window -- 7/8 on the first and on the last output row."""
    f = torch.ones(c.h // 2, dtype=dtype)
    f[0] -= 0.125
    f[-1] -= 0.125
    return f


def result(c, d, dtype=torch.float64, x_op=None, w_op=None):
    """The launch's output evaluated in `dtype` (B, Cout, h, w); x_op / w_op: the product's operands where they are not the inputs' own (emulations)."""
    xo = x_operand(c, d, dtype) if x_op is None else x_op.to(dtype)
    wm = weight_matrix(c, d["w"]).to(dtype) if w_op is None else w_op.to(dtype)
    y = torch.einsum("ok,bkhw->bohw", wm, xo)
    b = d["b"].to(dtype)[None, :, None, None]
    y = y + (b * row_factor(c, dtype)[None, None, :, None] if is_down(c) else b)
    if d["res"] is not None:
        y = d["res"].to(dtype) + y
    if d["scale"] is not None:
        y = y * d["scale"]
    return y


def weight_scale(w):
    """f16x2_weight_scale: the power of two that brings max|w| into [2^9, 2^10)."""
    return 2.0 ** (9 - math.floor(math.log2(w.abs().max().item())))


def f16_round_weights(w):
    """What the packer's h plane holds: RNE_f16(w s) / s (test_hip_fp16_mode.py)."""
    s = weight_scale(w)
    return (w.double() * s).half().double() / s


def one_plane_emulation(c, d):
    """fp64 product of the operands as the one-plane mode rounds them: RNE_f16 of the x operand -- whose fp64 value is exact in fp32 for every one-plane row
    here, so this is the kernel's single rounding -- and the h plane of the weights."""
    assert c.inst.nplk == 1 and not is_down(c)
    xo = x_operand(c, d, torch.float64)
    assert torch.equal(xo.float().double(), xo), "the x operand must be exact in fp32"
    return result(c, d, x_op=xo.float().half().double(), w_op=f16_round_weights(weight_matrix(c, d["w"])))


def references(c, d):
    """(fp64 truth, max error of the same expression in fp32 torch on the CPU)."""
    ref = result(c, d)
    return ref, (result(c, d, torch.float32).double() - ref).abs().max().item()


def stored(c, ref):
    """ref as the launch stores it: fp32, or fp16 (Y16) -- one rounding each from the exact value on the exact grid."""
    y = ref.float()
    return y.half() if c.inst.iom & 2 else y


# ---- the kernel's arithmetic in fp32 on the CPU (the exact grid's proof) -------------------------------------------------------------------
def split_f16x2(v):
    """(h, l) float32 of f16x2.h: h = RNE_f16(v), l = RNE_f16(2^11 (v - h))."""
    h = v.half().float()
    return h, ((v - h) * 2048.0).half().float()


def emulate(c, d, seed=5):
    """The kernel in fp32 torch: the x operand formed in fp32, both splits, one k at a time in a RANDOM order into the two fp32 accumulators (products of two
    fp16 numbers are exact in fp32: the only roundings are the additions'), conv_epilogue_wide's formula.  Returns (y as stored, share of nonzero l among
    the x operand's elements, largest sum_k |product| / grid over the outputs for the (h h, cross) accumulators, share of nonzero l among the weights)."""
    xo = x_operand(c, d, torch.float32)
    B, K, h, w = xo.shape
    xh, xl = split_f16x2(xo.permute(1, 0, 2, 3).reshape(K, -1))
    wm = weight_matrix(c, d["w"]).float()
    s = weight_scale(wm)
    wh, wl = split_f16x2(wm * s)
    acc = torch.zeros(c.cout, xh.shape[1])
    acl = torch.zeros_like(acc)
    for k in _gen(seed).permutation(K).tolist():
        if c.inst.nplk == 2:
            acl += wh[:, k, None] * xl[k]
            acl += wl[:, k, None] * xh[k]
        acc += wh[:, k, None] * xh[k]
    v = acc + acl * (1.0 / 2048.0) if c.inst.nplk == 2 else acc
    v = (v * (1.0 / s)).reshape(c.cout, B, h, w).permute(1, 0, 2, 3)
    b = d["b"][None, :, None, None]
    v = v + (b * row_factor(c, torch.float32)[None, None, :, None] if is_down(c) else b)
    if d["res"] is not None:
        v = d["res"] + v
    if d["scale"] is not None:
        v = v * d["scale"]
    sums = ((wh.abs().double() @ xh.abs().double()).max().item() / 2.0 ** -4,
            max((wh.abs().double() @ xl.abs().double()).max().item(), (wl.abs().double() @ xh.abs().double()).max().item()) / 2.0 ** 7)
    return (v.half() if c.inst.iom & 2 else v), (xl != 0).float().mean().item(), sums, (wl != 0).float().mean().item()


# ---- (d) the two-allocation input ----------------------------------------------------------------------------------------------------------
SEAMS = (8, 32, 40, 72)  # of Cin = 96: inside the first chunk, on a chunk boundary, inside the second, inside the third
SEAM_REFUSED = 20
CONCAT_MODES = {"split": (2, 0, 0), "split-affine": (2, 1, 0), "one-plane": (1, 0, 0), "one-plane-affine": (1, 1, 0), "io16": (1, 0, 3)}  # (pieces, prologue, io16)


def concat_case(cout, mode):
    pieces, pro, io16 = CONCAT_MODES[mode]
    inst = dispatch(96, cout, 8, 128, pieces, pro, io16, residual=io16 == 0, seam=8)
    return Case(inst, "ring", 96, cout, 8, 128, 2)
