// Post-processing of the segmentation labels (the reference's metrics/extractor/rangenet.py:197-405), gfx950.
//
//  knn_vote_kernel  the kNN label filter of RangeNet++ in one launch.  A block owns an 8 x 32 pixel tile, one pixel per thread.  The depth of
//                   the tile and of a halo of 2 (kh / 2) rows and 2 (kw / 2) columns -- dist_o(p) needs the jumps of p's neighbours, and those
//                   need THEIR neighbours' depths -- is read once into two LDS planes: the anchor value (a non-finite depth as -1) and the
//                   neighbour value (+inf where the anchor is negative, 0 outside the image); the labels with a halo of kh / 2, kw / 2 go to a
//                   third, as bytes.  Every dist_o is then one fp32 accumulator over the window, in row-major order, one rounding per
//                   operation (the __f*_rn intrinsics: nothing is contracted); a term outside the image is +0 and is skipped, which leaves
//                   the same bits.  The k <= 8 smallest are kept sorted in registers (insertion with a strict comparison, offsets ascending:
//                   ties go to the lowest offset), the vote is k^2 comparisons.  Nothing is written but the label, there are no atomics in
//                   the vote; the flag of an out-of-range label is an atomicOr of one bit by whoever sees it.
//  crf_iter_kernel  one mean-field iteration of the CRF-RNN.  Same tile.  Pass 1: every pixel of the tile and its kh / 2, kw / 2 halo gets the
//                   maximum and the sum of the softmax over the classes (LDS, with the mask and xyz).  Pass 2, class by class: the softmax
//                   plane S_c and S_c mask are staged in LDS (double-buffered: one barrier per class; the Q values of class c + 1 are loaded
//                   into registers before class c is summed and turned into the plane after it), a thread takes its two smoothness
//                   sums and the appearance sum over the window in row-major order, weighs them and adds compat[:, c] * that into one
//                   register accumulator per output class.  The appearance exponentials depend on the pixel pair only when theta_beta is the
//                   same for every class: they are then taken once, before the class loop, into registers (a statically indexed 7 x 7 array).
//                   fp32 throughout, expf of ordinary accuracy, a fixed order of every sum.
#include "common.h"

namespace r2dm {

namespace pp {
constexpr int TH = 8, TW = 32, THREADS = TH * TW;
constexpr int MAXK = 7, MAXR = MAXK / 2;          // window up to 7 x 7
constexpr int KNN_H = TH + 4 * MAXR, KNN_W = TW + 4 * MAXR;  // depth tile with the double halo
constexpr int HALO_H = TH + 2 * MAXR, HALO_W = TW + 2 * MAXR;  // tile with the single halo
constexpr int MAX_TOP = 8, MAX_CLASSES = 32;
}  // namespace pp

bool postproc_window_supported(int kh, int kw) { return kh >= 1 && kw >= 1 && kh <= pp::MAXK && kw <= pp::MAXK && (kh & 1) && (kw & 1); }

__global__ __launch_bounds__(pp::THREADS) void knn_vote_kernel(const float* __restrict__ depth, const long long* __restrict__ label,
                                                               const float* __restrict__ weight, long long* __restrict__ out, int H, int W, int kh,
                                                               int kw, int k, int classes, float cutoff, int* __restrict__ flag) {
    using namespace pp;
    __shared__ float sa[KNN_H * KNN_W];       // anchor depth
    __shared__ float sn[KNN_H * KNN_W];       // neighbour depth
    __shared__ signed char sl[HALO_H * HALO_W];
    __shared__ float sw[MAXK * MAXK];
    const int rh = kh / 2, rw = kw / 2;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const long img = (long)blockIdx.z * H * W;
    const int tid = threadIdx.x;
    const float inf = __builtin_inff();

    const int dh = TH + 4 * rh, dw = TW + 4 * rw;
    for (int i = tid; i < dh * dw; i += THREADS) {
        const int ly = i / dw, lx = i - ly * dw;
        const int gy = y0 - 2 * rh + ly, gx = x0 - 2 * rw + lx;
        float a = 0.f, n = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            a = depth[img + (long)gy * W + gx];
            if (!(__builtin_fabsf(a) < inf)) a = -1.f;  // NaN, +inf, -inf: the invalid marker
            n = a < 0.f ? inf : a;
        }
        sa[ly * KNN_W + lx] = a;
        sn[ly * KNN_W + lx] = n;
    }
    const int lh = TH + 2 * rh, lw = TW + 2 * rw;
    bool bad = false;
    for (int i = tid; i < lh * lw; i += THREADS) {
        const int ly = i / lw, lx = i - ly * lw;
        const int gy = y0 - rh + ly, gx = x0 - rw + lx;
        int l = 0;  // the padding of the label image
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const long long v = label[img + (long)gy * W + gx];
            if (v < 0 || v >= classes) l = -1, bad = true;
            else l = (int)v;
        }
        sl[ly * HALO_W + lx] = (signed char)l;
    }
    if (bad) atomicOr(flag, 1);
    if (tid < kh * kw) sw[tid] = weight[tid];
    __syncthreads();

    const int ty = tid / TW, tx = tid - ty * TW;
    const int gy = y0 + ty, gx = x0 + tx;
    if (gy >= H || gx >= W) return;

    // the window offsets q for which p + q is inside the image (the others add +0)
    const int qy0 = max(0, rh - gy), qy1 = min(kh, H - gy + rh);
    const int qx0 = max(0, rw - gx), qx1 = min(kw, W - gx + rw);

    float bd[MAX_TOP];
    int bl[MAX_TOP];  // the winner's label; -2: the slot is empty
#pragma unroll
    for (int j = 0; j < MAX_TOP; ++j) bd[j] = 0.f, bl[j] = -2;

    for (int oy = 0; oy < kh; ++oy) {
        for (int ox = 0; ox < kw; ++ox) {
            float acc = 0.f;
            for (int qy = qy0; qy < qy1; ++qy) {
                const float* pa = sa + (ty + rh + qy) * KNN_W + tx + rw;         // depth(p + q), q = (qy - rh, qx - rw)
                const float* pn = sn + (ty + qy + oy) * KNN_W + tx + ox;         // n(p + q + o)
                for (int qx = qx0; qx < qx1; ++qx)
                    acc = __fadd_rn(acc, __fmul_rn(sw[qy * kw + qx], __builtin_fabsf(__fsub_rn(pn[qx], pa[qx]))));
            }
            const int lab = sl[(ty + oy) * HALO_W + tx + ox];
            // before slot j: the slot is empty, or acc < its distance (a NaN is the largest and never precedes anything)
            bool before[MAX_TOP];
#pragma unroll
            for (int j = 0; j < MAX_TOP; ++j) before[j] = bl[j] == -2 || acc < bd[j] || (bd[j] != bd[j] && acc == acc);
#pragma unroll
            for (int j = MAX_TOP - 1; j >= 0; --j) {
                if (j < k && before[j]) {
                    if (j > 0 && before[j - 1]) bd[j] = bd[j - 1], bl[j] = bl[j - 1];
                    else bd[j] = acc, bl[j] = lab;
                }
            }
        }
    }

    // the vote: a winner beyond the cutoff or with an out-of-range label (-1) votes for nothing
    int vote[MAX_TOP];
#pragma unroll
    for (int j = 0; j < MAX_TOP; ++j) vote[j] = (j < k && bl[j] >= 0 && !(cutoff > 0.f && bd[j] > cutoff)) ? bl[j] : -1;
    int best = 0, best_n = 0;
#pragma unroll
    for (int j = 0; j < MAX_TOP; ++j) {
        int n = 0;
#pragma unroll
        for (int i = 0; i < MAX_TOP; ++i) n += (vote[i] == vote[j]) ? 1 : 0;
        if (vote[j] >= 0 && (n > best_n || (n == best_n && vote[j] < best))) best = vote[j], best_n = n;
    }
    out[img + (long)gy * W + gx] = best;
}

hipError_t launch_knn_vote(const float* depth, const long long* label, const float* weight, long long* out, int B, int H, int W, int kh, int kw, int k,
                           int classes, float cutoff, int* flag, hipStream_t s) {
    using namespace pp;
    if (!postproc_window_supported(kh, kw) || k < 1 || k > MAX_TOP || k > kh * kw || classes < 1 || classes > MAX_CLASSES || B < 1 || B > 65535 ||
        H < 1 || W < 1)
        return hipErrorInvalidValue;
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, B);
    if (grid.y > 65535) return hipErrorInvalidValue;
    knn_vote_kernel<<<grid, THREADS, 0, s>>>(depth, label, weight, out, H, W, kh, kw, k, classes, cutoff, flag);
    return hipGetLastError();
}

__global__ __launch_bounds__(pp::THREADS) void crf_iter_kernel(const float* __restrict__ qin, const float* __restrict__ unary,
                                                               const float* __restrict__ xyz, const float* __restrict__ mask,
                                                               const float* __restrict__ params, float* __restrict__ qout, int N, int H, int W, int kh,
                                                               int kw, int uniform_beta) {
    using namespace pp;
    constexpr int P = HALO_H * HALO_W;
    __shared__ float smax[P], sinv[P], smask[P], sxyz[3][P];
    __shared__ float splane[2][2][P];  // [buffer][S, S mask]
    const int rh = kh / 2, rw = kw / 2, K = kh * kw;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const long hw = (long)H * W;
    const int b = blockIdx.z;
    const int tid = threadIdx.x;
    const float* q = qin + (long)b * N * hw;
    const float* kgamma = params;
    const float* kalpha = kgamma + N * K;
    const float* ws = kalpha + N * K;
    const float* wa = ws + N;
    const float* beta = wa + N;
    const float* compat = beta + N;

    // pass 1: softmax statistics, the mask and xyz of the tile and its halo (zeros outside the image)
    const int lh = TH + 2 * rh, lw = TW + 2 * rw;
    for (int i = tid; i < lh * lw; i += THREADS) {
        const int ly = i / lw, lx = i - ly * lw;
        const int gy = y0 - rh + ly, gx = x0 - rw + lx;
        const int li = ly * HALO_W + lx;
        float mx = 0.f, inv = 0.f, m = 0.f, px = 0.f, py = 0.f, pz = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const long g = (long)gy * W + gx;
            mx = q[g];
            for (int c = 1; c < N; ++c) mx = fmaxf(mx, q[c * hw + g]);
            float sum = 0.f;
            for (int c = 0; c < N; ++c) sum += expf(q[c * hw + g] - mx);
            inv = 1.0f / sum;
            m = mask[b * hw + g];
            px = xyz[(b * 3L + 0) * hw + g], py = xyz[(b * 3L + 1) * hw + g], pz = xyz[(b * 3L + 2) * hw + g];
        }
        smax[li] = mx, sinv[li] = inv, smask[li] = m;
        sxyz[0][li] = px, sxyz[1][li] = py, sxyz[2][li] = pz;
    }
    // Staging of a class plane, split in two so that the loads of class c + 1 fly while class c is summed: fetch() reads the thread's (up to
    // STAGE) halo pixels of Q into registers, store() turns them into S and S mask in LDS.  Outside the image the offset is -1 and the value 0:
    // with max = 0 and inv = 0 from pass 1, S = exp(0 - 0) * 0 = 0 there, the zero padding of the convolution and of unfold.
    constexpr int STAGE = (P + THREADS - 1) / THREADS;
    long goff[STAGE];
    int loff[STAGE];
#pragma unroll
    for (int r = 0; r < STAGE; ++r) {
        const int i = tid + r * THREADS;
        goff[r] = -1, loff[r] = -1;
        if (i < lh * lw) {
            const int ly = i / lw, lx = i - ly * lw;
            const int gy = y0 - rh + ly, gx = x0 - rw + lx;
            loff[r] = ly * HALO_W + lx;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) goff[r] = (long)gy * W + gx;
        }
    }
    float qreg[STAGE];
    auto fetch = [&](int c) {
#pragma unroll
        for (int r = 0; r < STAGE; ++r) qreg[r] = goff[r] >= 0 ? q[c * hw + goff[r]] : 0.f;
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int r = 0; r < STAGE; ++r)
            if (loff[r] >= 0) {
                const float s = expf(qreg[r] - smax[loff[r]]) * sinv[loff[r]];
                splane[buf][0][loff[r]] = s;
                splane[buf][1][loff[r]] = s * smask[loff[r]];
            }
    };
    __syncthreads();
    fetch(0);
    store(0);

    const int ty = tid / TW, tx = tid - ty * TW;
    const int gy = y0 + ty, gx = x0 + tx;
    const bool live = gy < H && gx < W;
    const int lc = (ty + rh) * HALO_W + tx + rw;  // the thread's own pixel in the halo tile

    // the appearance term per neighbour: exp(-d2 / beta) if theta_beta is uniform, else d2 (the exponential is then taken per class)
    float app[MAXK][MAXK];
    {
        const float ax = sxyz[0][lc], ay = sxyz[1][lc], az = sxyz[2][lc];
        const float b0 = beta[0];
#pragma unroll
        for (int oy = 0; oy < MAXK; ++oy)
#pragma unroll
            for (int ox = 0; ox < MAXK; ++ox) {
                float v = 0.f;
                if (oy < kh && ox < kw) {
                    const int li = (ty + oy) * HALO_W + tx + ox;
                    const float dx = sxyz[0][li] - ax, dy = sxyz[1][li] - ay, dz = sxyz[2][li] - az;
                    const float d2 = dx * dx + dy * dy + dz * dz;
                    v = uniform_beta ? expf(-d2 / b0) : d2;
                }
                app[oy][ox] = v;
            }
    }
    const float mc = smask[lc];

    float pw[MAX_CLASSES];
#pragma unroll
    for (int j = 0; j < MAX_CLASSES; ++j) pw[j] = 0.f;

    for (int c = 0; c < N; ++c) {
        __syncthreads();  // plane c is staged; plane c - 1 has been read by everyone
        if (c + 1 < N) fetch(c + 1);
        const float* S = splane[c & 1][0];
        const float* SM = splane[c & 1][1];
        const float* kg = kgamma + c * K;
        const float* ka = kalpha + c * K;
        const float bc = beta[c];
        float sg = 0.f, sal = 0.f, ap = 0.f;
#pragma unroll
        for (int oy = 0; oy < MAXK; ++oy)
#pragma unroll
            for (int ox = 0; ox < MAXK; ++ox) {
                if (oy < kh && ox < kw && !(oy == rh && ox == rw)) {
                    const int li = (ty + oy) * HALO_W + tx + ox;
                    const float s = S[li];
                    sg += kg[oy * kw + ox] * s;
                    sal += ka[oy * kw + ox] * s;
                    ap += SM[li] * (uniform_beta ? app[oy][ox] : expf(-app[oy][ox] / bc));
                }
            }
        const float wk = ws[c] * sg + wa[c] * ((ap * mc) * sal);
#pragma unroll
        for (int j = 0; j < MAX_CLASSES; ++j)
            if (j < N) pw[j] += compat[j * N + c] * wk;
        if (c + 1 < N) store((c + 1) & 1);
    }
    if (!live) return;
    const long g = (long)b * N * hw + (long)gy * W + gx;
#pragma unroll
    for (int j = 0; j < MAX_CLASSES; ++j)
        if (j < N) qout[g + j * hw] = unary[g + j * hw] - pw[j];
}

hipError_t launch_crf_iter(const float* q_in, const float* unary, const float* xyz, const float* mask, const float* params, float* q_out, int B, int N,
                           int H, int W, int kh, int kw, int uniform_beta, hipStream_t s) {
    using namespace pp;
    if (!postproc_window_supported(kh, kw) || N < 1 || N > MAX_CLASSES || B < 1 || B > 65535 || H < 1 || W < 1) return hipErrorInvalidValue;
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, B);
    if (grid.y > 65535) return hipErrorInvalidValue;
    crf_iter_kernel<<<grid, THREADS, 0, s>>>(q_in, unary, xyz, mask, params, q_out, N, H, W, kh, kw, uniform_beta);
    return hipGetLastError();
}

}  // namespace r2dm
