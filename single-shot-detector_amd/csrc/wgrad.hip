// The weight gradient of a k x k convolution (k = 1 or 3, stride 1 or 2) on the exact-fp32 matrix instruction
// (v_mfma_f32_32x32x2_f32):
//     dw[tap][ci][co] = sum over levels, images and output positions r of  x[the tap's input position of r][ci] * dy[r][co]
// a GEMM with M = k*k * Cin, N = Cout and K = every output position of every level.  x and dy are the caller's LOGICAL NHWC
// tensors (the sum runs over positions, so the channel order of the activations plays no part); the tap shift, the stride and the
// zero border are in the loads of x, as in the forward.  M x N gives few tiles, so K is cut into slices of `rows_per_slice`
// positions (a slice never crosses a level): one block per (slice, tile) writes its partial tile to the workspace, and
// wgrad_reduce adds the slices of an element in ascending slice order, which is ascending level order.  No atomics: two
// runs give the same bits.  The order of the sum (include/ssd_hip.h, "the TRAIN head") is this kernel's, not an oracle's.
#include "train_head.h"

typedef float v16f __attribute__((ext_vector_type(16)));

static __device__ inline unsigned wg_udiv(unsigned n, UDiv d) { return d.sh < 0 ? n : (__umulhi(n, d.mag) >> d.sh); }

#define WG_BK 16          // positions per K-step

// Block tile 128 (ci of one tap) x BN (co), BN = 32 * NJ * WN; 4 waves as WM x WN, each NI x NJ accumulators of 32 x 32.
template <int NI, int NJ, int WM, int WN>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradArgs a)
{
    constexpr int BM = 32 * NI * WM, BN = 32 * NJ * WN;
    static_assert(BM == 128 && WM * WN == 4, "four waves, 128 input channels per tile");
    constexpr int AS = BM + 32, BS = BN + 32;              // row strides, + 32 floats: 160 is a multiple of the 32 banks, so the rows k and k + 1 that a wave reads start on
                                                           // the SAME bank; the read is conflict-free because a 64-lane ds_read_b32 is served as two half-waves of 32 consecutive floats
    __shared__ float As[WG_BK * AS];
    __shared__ float Bs[WG_BK * BS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slice = blockIdx.x;
    int l = 0;
    while (l + 1 < a.nlevels && slice >= a.lv[l + 1].slice_begin) ++l;
    const WgradLevel &L = a.lv[l];
    const int tap = blockIdx.z / a.tiles_ci, ci0 = (blockIdx.z % a.tiles_ci) * BM, co0 = blockIdx.y * BN;
    const int kh = tap / a.k - a.pad, kw = tap % a.k - a.pad;      // the tap's offset from the output position's first input
    const int r_begin = (slice - L.slice_begin) * a.rows_per_slice;
    const int r_end = min(L.R, r_begin + a.rows_per_slice);
    const int vx = th_width(a.Cin), vy = th_width(a.Cout);      // C % 4 == 2 (ShuffleNet's 58): 8-byte loads

    // staging: thread -> (row k = tid / 32 (+ 8), channel quad tid % 32) of the x tile; the dy tile likewise over BN / 4 quads
    const int ak = tid >> 5, ac = (tid & 31) << 2;
    constexpr int BQ = BN / 4, BROWS = 256 / BQ, BPASS = (WG_BK + BROWS - 1) / BROWS;
    const int bk = tid / BQ, bc = (tid % BQ) << 2;
    v4f xa[2], yb[BPASS];
    auto fetch = [&](int r0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int r = r0 + ak + 8 * p;
            v4f v = {0.f, 0.f, 0.f, 0.f};
            if (r < r_end) {
                const unsigned img = wg_udiv((unsigned)r, L.dP), rem = (unsigned)r - img * (unsigned)L.P;
                const int oy = (int)wg_udiv(rem, L.dOW), ox = (int)rem - oy * L.OW;
                const int sy = oy * a.stride + kh, sx = ox * a.stride + kw;
                if (sy >= 0 && sy < L.H && sx >= 0 && sx < L.W)
                    v = th_load4(L.x + (((long long)img * L.H + sy) * L.W + sx) * a.Cin, ci0 + ac, a.Cin, vx);
            }
            xa[p] = v;
        }
#pragma unroll
        for (int p = 0; p < BPASS; ++p) {
            const int k = bk + BROWS * p, r = r0 + k;
            v4f v = {0.f, 0.f, 0.f, 0.f};
            if (k < WG_BK && r < r_end) v = th_load4(L.dy + (long long)r * a.Cout, co0 + bc, a.Cout, vy);
            yb[p] = v;
        }
    };

    v16f acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    const int m0 = (wave / WN) * (32 * NI), n0 = (wave % WN) * (32 * NJ);
    const int lk = lane >> 5, li = lane & 31;

    fetch(r_begin);
    for (int r0 = r_begin; r0 < r_end; r0 += WG_BK) {
        __syncthreads();                                   // the previous step's reads of As / Bs are done
#pragma unroll
        for (int p = 0; p < 2; ++p) *(v4f *)(As + (ak + 8 * p) * AS + ac) = xa[p];
#pragma unroll
        for (int p = 0; p < BPASS; ++p)
            if (bk + BROWS * p < WG_BK) *(v4f *)(Bs + (bk + BROWS * p) * BS + bc) = yb[p];
        __syncthreads();
        if (r0 + WG_BK < r_end) fetch(r0 + WG_BK);         // the next step's loads fly under this step's MFMAs
#pragma unroll
        for (int kk = 0; kk < WG_BK / 2; ++kk) {
            const int k = 2 * kk + lk;
            float af[NI], bf[NJ];
#pragma unroll
            for (int i = 0; i < NI; ++i) af[i] = As[k * AS + m0 + 32 * i + li];
#pragma unroll
            for (int j = 0; j < NJ; ++j) bf[j] = Bs[k * BS + n0 + 32 * j + li];
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }
    // accumulator element e of a lane: row 8 * (e / 4) + 4 * (lane / 32) + e % 4, column lane % 32
    float *part = a.partial + ((long long)slice * a.k * a.k + tap) * a.Cin * a.Cout;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int co = co0 + n0 + 32 * j + li;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ci = ci0 + m0 + 32 * i + 8 * (e >> 2) + 4 * lk + (e & 3);
                if (ci < a.Cin && co < a.Cout) part[(long long)ci * a.Cout + co] = acc[i][j][e];
            }
        }
}

// dw[i] = partial[0][i] + partial[1][i] + ... in ascending slice order, one fp32 addition at a time
__global__ __launch_bounds__(256) void wgrad_reduce(const float *partial, int n_slices, long long count, float *dw)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    float s = partial[i];
    for (int k = 1; k < n_slices; ++k) s = s + partial[(long long)k * count + i];
    dw[i] = s;
}

int wgrad_tile_n(int Cout) { return Cout <= 32 ? 32 : 128; }

hipError_t launch_wgrad(const WgradArgs &a, float *dw, hipStream_t s)
{
    const int BN = wgrad_tile_n(a.Cout);
    const dim3 grid((unsigned)a.n_slices, (unsigned)((a.Cout + BN - 1) / BN), (unsigned)(a.k * a.k * a.tiles_ci));
    if (BN == 32) hipLaunchKernelGGL((wgrad_kernel<1, 1, 4, 1>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((wgrad_kernel<2, 2, 2, 2>), grid, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long count = (long long)a.k * a.k * a.Cin * a.Cout;
    hipLaunchKernelGGL(wgrad_reduce, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, a.partial, a.n_slices, count, dw);
    return hipGetLastError();
}
