// The class logits (256 -> 6 * num_classes, 3x3, all five levels) without computing them all: the post-processing reads only
// the octets of 8 consecutive logits that hold a value at or above the conservative logit bound (PostArgs::scan_bits), about
// one octet in a thousand.  Four launches on the class tower's stream (DESIGN 4.2 has the derivation of the bound):
//
//   convert   the class tower's last output (fp32 rows, x >= 0 behind its ReLU) -> one f16 plane xu >= x, rounded UP and never
//             subnormal (0 < x < 2^-14 -> 2^-14); x < 0 or NaN -> NaN, which marks.
//   screen    implicit GEMM on v_mfma_f32_32x32x16_f16: P = sum xu * Wp, N = sum xu * Wn with Wp >= max(w, 0) rounded up and
//             Wn <= max(-w, 0) rounded down (both never subnormal; weights.hip packs them).  Every term of either sum is
//             non-negative, so ANY summation order and rounding of the matrix pipe is within a relative n * u' of the sum, and
//                 U = P (1 + 2^-9) - N (1 - 2^-9) + cst + 2^-18 (P + N + |cst|),   cst >= bias + 2^-14 sum Wn + 2^-20 |bias|
//             is an upper bound of the exact fp32 logit.  The octet's bit is set unless U < scan_lo (written !(U < lo): NaN and
//             inf mark).  Tile 256 rows x 128 logit columns per block: waves (m, 0) hold P, waves (m, 1) hold N of the same 128
//             columns.  For every (k, column) at most one of Wp, Wn is non-zero, so the B tile is ONE signed plane (Wp as it
//             is, Wn with the sign bit set, never -0) of 128 rows that both waves of a pair read; each takes its operand
//             with integer operations on the halves (screen_operand).  Staging as igemm16.hip: LDS-DMA, XOR-swizzled 128-B
//             rows (here 64 channels of f16), zero padding = the buffer range check; a ring of three stages of 48 KB with
//             counted waits, fragments of the next 16-channel step read under the MFMAs of this one.  Block 0 also zeroes
//             the row lists' counters.
//   compact   bitmap -> per column octet the list of marked rows (one LDS counter set per block, one global add per block and
//             column octet).
//   fill      per marked octet the 8 logits EXACTLY: acc = fmaf(x_k, w_k, acc) from +0 over k = tap-major, then logical input
//             channel ascending (padded taps as zero operands), then acc + bias -- the chain and the epilogue of the dense
//             kernel (igemm.hip MODE 4) and of the oracle.  A block owns one column octet: its 2304 x 8 weights are staged in
//             LDS once, the input patches stream; 8 lanes per item, one per logit.
#include "ssd_internal.h"
#include <type_traits>

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef short v2s __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void *lds_ptr_t;

// the screen's LDS ring: a stage is a 256-row A tile + a 128-row B tile of 128-B rows
#define SCREEN_STAGE_BYTES ((256 + 128) * 128)
#define SCREEN_STAGES 3

// x >= 0 -> the smallest normal f16 (or inf) that is >= x, 0 for 0; anything else (x < 0, NaN) -> NaN
__device__ __forceinline__ unsigned f16_up_bits(float x)
{
    if (!(x >= 0.0f)) return 0x7e00u;
    if (x == 0.0f) return 0u;
    const _Float16 h = (_Float16)x;
    unsigned b = (unsigned)__builtin_bit_cast(unsigned short, h);
    if ((float)h < x) b += 1u;              // (positive: the next bit pattern is the next value, 0x7bff + 1 = inf)
    return b < 0x0400u ? 0x0400u : b;
}

__global__ __launch_bounds__(256) void logit_convert_kernel(const float *__restrict__ x, unsigned short *__restrict__ x16, long long n8)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        const v4f a = *(const v4f *)(x + i * 8), b = *(const v4f *)(x + i * 8 + 4);
        v4u o;
        o[0] = f16_up_bits(a[0]) | (f16_up_bits(a[1]) << 16);
        o[1] = f16_up_bits(a[2]) | (f16_up_bits(a[3]) << 16);
        o[2] = f16_up_bits(b[0]) | (f16_up_bits(b[1]) << 16);
        o[3] = f16_up_bits(b[2]) | (f16_up_bits(b[3]) << 16);
        *(v4u *)(x16 + i * 8) = o;
    }
}

// the level of a tile / of a row, copied field by field from constant indices: the kernel arguments stay scalar loads
__device__ __forceinline__ ScreenLevel screen_level_of_tile(const ScreenArgs &a, int tile_m)
{
    ScreenLevel L = a.lv[0];
#pragma unroll
    for (int i = 1; i < SCREEN_MAX_LEVELS; ++i)
        if (i < a.nlevels && tile_m >= a.lv[i].tile_begin) L = a.lv[i];
    return L;
}
__device__ __forceinline__ ScreenLevel screen_level_of_row(const ScreenArgs &a, int r)
{
    ScreenLevel L = a.lv[0];
#pragma unroll
    for (int i = 1; i < SCREEN_MAX_LEVELS; ++i)
        if (i < a.nlevels && r >= a.lv[i].row_begin) L = a.lv[i];
    return L;
}

// the operand of a wave from a fragment of the signed plane, on the 16-bit halves as integers: sgn = 0 keeps the halves with
// the sign clear (Wp: a NaN stays a NaN), sgn = 0x80008000 flips the signs first and so keeps the magnitudes of the others
// (Wn); everything else becomes +0.  (A floating-point max would drop the NaNs.)
__device__ __forceinline__ v8h screen_operand(v4u f, unsigned sgn)
{
    v4u o;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const v2s h = __builtin_bit_cast(v2s, f[d] ^ sgn);
        o[d] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(h, v2s{0, 0}));
    }
    return __builtin_bit_cast(v8h, o);
}

__global__ __launch_bounds__(256, 1) void logit_screen_kernel(const ScreenArgs a)
{
    constexpr int BM = 256;
    constexpr int A_BYTES = BM * 128;
    constexpr int STAGE = SCREEN_STAGE_BYTES;       // 32 KB A + 16 KB B
    constexpr int NSTAGE = SCREEN_STAGES;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (uniform: the LDS-DMA's base and the wave's role are scalars)
    const int wave_m = wave >> 1, wave_n = wave & 1;
    const unsigned sgn = wave_n ? 0x80008000u : 0u;                 // waves (m, 0) take Wp, waves (m, 1) Wn of the same fragments
    int swz;
    {   // blocks b, b+8, ... share an XCD: consecutive tiles per XCD (bijective remap, as igemm16.hip)
        const int nblk = gridDim.x, bid = blockIdx.x;
        const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7;
        swz = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int tile_n = swz % a.NT;
    const int tile_m = swz / a.NT;
    const ScreenLevel L = screen_level_of_tile(a, tile_m);
    const int H = L.H, W = L.W, P = L.P, M = L.M;
    const int Cin = a.Cin;
    const int m0 = (tile_m - L.tile_begin) * BM;

    const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(a.x16 + L.in_off), 0, (int)((long long)a.B * P * Cin * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t brsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)a.w16, 0, (int)((long long)9 * a.NT * 128 * Cin * 2), 0x00020000);
    constexpr unsigned OOB = 0x80000000u;

    // DMA bookkeeping (igemm16.hip): wave w stages rows w*64 .. w*64+63 of the A tile and rows w*32 .. w*32+31 of the B tile,
    // 8 rows per instruction: lane -> row (lane >> 3), LDS slot (lane & 7), source chunk slot ^ ((row >> 1) & 7)
    int abase[8], aiy0[8], aix0[8];
    int boff[4];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int row = wave * 64 + u * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ ((row >> 1) & 7);
        const int m = m0 + row;
        const bool rowok = m < M;
        const int mm = rowok ? m : 0;
        const int b = mm / P, p = mm - b * P;
        const int oy = p / W, ox = p - oy * W;
        abase[u] = b * P * Cin * 2 + chunk * 16;
        aiy0[u] = rowok ? oy - 1 : -(1 << 20);
        aix0[u] = ox - 1;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int row = wave * 32 + u * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ ((row >> 1) & 7);
        boff[u] = (tile_n * 128 + row) * Cin * 2 + chunk * 16;
    }
    const int b_tapstride = a.NT * 128 * Cin * 2;
    const int KC = Cin >> 6;
    const int KS = 9 * KC;
    // K order: 64-channel block outer, filter tap inner (the bound does not depend on the order): the nine taps of a block
    // re-read the same lines nine K-steps apart -> L2 hits.  12 DMA instructions per wave and K-step; (dtap, dkc) is the K-step
    // the next call stages.  Past the last K-step the same 12 instructions are issued with every offset out of range (they
    // fetch nothing and write zeros into a stage nobody reads again): the loop below stays free of branches and its counted
    // wait stays right to the end.
    int dtap = 0, dkc = 0;
    auto dma = [&](int stage_off) {
        const bool live = dkc < KC;
        const int tky = dtap / 3, tkx = dtap - 3 * tky;
        unsigned char *abuf = lds + stage_off + wave * 64 * 128;
        unsigned char *bbuf = lds + stage_off + A_BYTES + wave * 32 * 128;
        const int so = dkc * 128, bso = dtap * b_tapstride + dkc * 128;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int iy = aiy0[u] + tky, ix = aix0[u] + tkx;
            const bool ok = live & ((unsigned)iy < (unsigned)H) & ((unsigned)ix < (unsigned)W);
            const unsigned off = ok ? (unsigned)(abase[u] + (iy * W + ix) * Cin * 2) : OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(arsrc, (lds_ptr_t)(abuf + u * 1024), 16, (int)off, so, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(brsrc, (lds_ptr_t)(bbuf + u * 1024), 16, live ? boff[u] : (int)OOB, bso, 0, 0);
        if (++dtap == 9) { dtap = 0; ++dkc; }
    };
    // fragments of the 16-channel step s: lane group (lane >> 5) takes chunk 2s + group of its row
    int roff[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int chunk = 2 * s + (lane >> 5);
        roff[s] = (lane & 31) * 128 + ((chunk ^ (((lane & 31) >> 1) & 7)) << 4);
    }
    auto rd = [&](int stage_off, int s, v4f (&fa)[4], v4u (&fb)[4]) {
        const unsigned char *ab = lds + stage_off + wave_m * 4 * 4096;
        const unsigned char *bb = lds + stage_off + A_BYTES;
#pragma unroll
        for (int i = 0; i < 4; ++i) fa[i] = *(const v4f *)(ab + i * 4096 + roff[s]);
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = *(const v4u *)(bb + j * 4096 + roff[s]);
    };
    v16f acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    auto mf = [&](const v4f (&fa)[4], const v4u (&fb)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const v8h bj = screen_operand(fb[j], sgn);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, fa[i]), bj, acc[i][j], 0, 0, 0);
        }
    };
    // 16 MFMAs with the 8 fragment reads of the next 16-channel step (a ds_read_b128 of the four waves together is about one
    // MFMA long) and the operand selects between them; with_dma: the 12 DMA pieces of a K-step as well
    auto sched = [&](bool with_dma) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (i < 8) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            if (with_dma && i >= 4) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            if (with_dma) __builtin_amdgcn_sched_group_barrier(0x006, 8, 0);
            else __builtin_amdgcn_sched_group_barrier(0x006, 4, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    // A ring of three stages.  The barrier of K-step ks sits before its last 16-channel step: every fragment of stage ks is in
    // registers by then (lgkmcnt(0)) and every wave's share of stage ks + 1 has landed (vmcnt: only the 12 pieces of K-step
    // ks + 2 may be outstanding), so behind it the first fragments of K-step ks + 1 are read and stage ks is refilled with
    // K-step ks + 3 -- a fill has two K-steps to land, up to 96 KB are in flight.
    v4f fa0[4], fa1[4];
    v4u fb0[4], fb1[4];
    int cur = 0, nxt = STAGE, nn = 2 * STAGE;
    static_assert(NSTAGE == 3, "the ring below rotates three stages");
    dma(cur);
    dma(nxt);
    dma(nn);
    asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    rd(cur, 0, fa0, fb0);
#pragma unroll 1
    for (int ks = 0; ks < KS; ++ks) {
        rd(cur, 1, fa1, fb1);
        mf(fa0, fb0);
        sched(false);
        rd(cur, 2, fa0, fb0);
        mf(fa1, fb1);
        sched(false);
        rd(cur, 3, fa1, fb1);
        mf(fa0, fb0);
        sched(false);
        asm volatile("s_waitcnt vmcnt(12) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        rd(nxt, 0, fa0, fb0);       // (behind the last K-step: a stage that is not used)
        dma(cur);
        mf(fa1, fb1);
        sched(true);
        const int t = cur;
        cur = nxt; nxt = nn; nn = t;
    }

    // ---- epilogue, 32 rows of the wave's sub-tile per pass: every wave puts its sums into LDS ([r][j][lane]: the P wave and
    // the N wave of a pair hold the same row and column in the same lane and register), then each wave of the pair forms U
    // for half of the registers and marks.  acc[i][j][r]: row i*32 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column j*32 + (lane & 31).
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    // the row lists' counters of the compaction launch behind this one (no DMA is outstanding any more: nothing counts vmcnt here)
    if (blockIdx.x == 0 && tid < (a.Cout >> 3)) a.counts[tid] = 0;
    float *mine = (float *)lds + wave * 4096;
    const float *Pp = (const float *)lds + (wave_m * 2) * 4096, *Np = Pp + 4096;
    float cst[4];
    bool colok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = tile_n * 128 + j * 32 + (lane & 31);
        colok[j] = col < a.Cout;
        cst[j] = colok[j] ? a.cst[col] : 0.0f;
    }
    const float lo = a.lo;
    const int rstride = a.out_rstride;
    const long long bstride = a.out_bstride, out_off = L.out_off;
    auto pass = [&](auto itag) __attribute__((always_inline)) {       // (a constant i: the accumulators stay registers)
        constexpr int i = decltype(itag)::value;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) mine[(r * 4 + j) * 64 + lane] = acc[i][j][r];
        __syncthreads();
        const int rbase = m0 + wave_m * 128 + i * 32;
#pragma unroll 1
        for (int r = wave_n * 8; r < wave_n * 8 + 8; ++r) {
            const int rowl = rbase + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float Pv = Pp[(r * 4 + j) * 64 + lane], Nv = Np[(r * 4 + j) * 64 + lane];
                const float t1 = Pv * 1.001953125f, t2 = Nv * 0.998046875f;
                const float U = ((t1 - t2) + cst[j]) + 3.814697265625e-06f * ((Pv + Nv) + __builtin_fabsf(cst[j]));
                const bool flag = colok[j] && rowl < M && !(U < lo);
                const unsigned long long mask = __ballot(flag);
                if (mask != 0ull && lane < 8) {
                    // lane q: byte q of the mask = the 8 columns of octet (q & 3) in row half (q >> 2)
                    const unsigned byte = (unsigned)(mask >> (8 * lane)) & 0xffu;
                    const int row = rbase + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 2);
                    const int col8 = tile_n * 128 + j * 32 + (lane & 3) * 8;
                    if (byte && row < M && col8 < a.Cout) {
                        const int b = row / P, p = row - b * P;
                        const unsigned oct = (unsigned)((out_off + (long long)b * bstride + (long long)p * rstride + col8) >> 3);
                        atomicOr(a.bits + (oct >> 5), 1u << (oct & 31));
                    }
                }
            }
        }
        __syncthreads();
    };
    pass(std::integral_constant<int, 0>{});
    pass(std::integral_constant<int, 1>{});
    pass(std::integral_constant<int, 2>{});
    pass(std::integral_constant<int, 3>{});
}

// bitmap -> lists[o][0 .. counts[o]): the marked rows (global row index over the levels) of column octet o
__global__ __launch_bounds__(256) void logit_compact_kernel(const ScreenArgs a, long long nwords)
{
    __shared__ int lcnt[SCREEN_MAX_OCT], lbase[SCREEN_MAX_OCT];
    __shared__ unsigned short slot[256 * 32];
    const int NO = a.Cout >> 3;
    const unsigned NC = (unsigned)a.out_bstride;                    // logits per image
    for (long long w0 = (long long)blockIdx.x * 256; w0 < nwords; w0 += (long long)gridDim.x * 256) {
        const long long w = w0 + threadIdx.x;
        const unsigned bits = w < nwords ? a.bits[w] : 0u;
        if (!__syncthreads_or(bits != 0u)) continue;
        if ((int)threadIdx.x < NO) lcnt[threadIdx.x] = 0;
        __syncthreads();
        auto decode = [&](int bpos, int &o) -> int {
            const unsigned e = ((unsigned)w * 32u + (unsigned)bpos) * 8u;       // first logit of the octet in [B][N][C]
            const unsigned b = e / NC, rem = e - b * NC;
            int lvl = 0;
#pragma unroll
            for (int i = 1; i < SCREEN_MAX_LEVELS; ++i)
                if (i < a.nlevels && rem >= (unsigned)a.lv[i].out_off) lvl = i;
            const unsigned within = rem - (unsigned)a.lv[lvl].out_off;
            const unsigned p = within / (unsigned)a.out_rstride;
            o = (int)((within - p * (unsigned)a.out_rstride) >> 3);
            return a.lv[lvl].row_begin + (int)b * a.lv[lvl].P + (int)p;
        };
        for (unsigned rest = bits; rest; rest &= rest - 1) {
            const int bpos = __builtin_ctz(rest);
            int o;
            (void)decode(bpos, o);
            slot[threadIdx.x * 32 + bpos] = (unsigned short)atomicAdd(&lcnt[o], 1);       // (LDS; at most 256 * 32 per block)
        }
        __syncthreads();
        if ((int)threadIdx.x < NO) lbase[threadIdx.x] = lcnt[threadIdx.x] ? atomicAdd(a.counts + threadIdx.x, lcnt[threadIdx.x]) : 0;
        __syncthreads();
        for (unsigned rest = bits; rest; rest &= rest - 1) {
            const int bpos = __builtin_ctz(rest);
            int o;
            const int row = decode(bpos, o);
            a.lists[(long long)o * a.rows_total + lbase[o] + slot[threadIdx.x * 32 + bpos]] = row;
        }
        __syncthreads();
    }
}

// Work unit: a chunk of up to FILL_CHUNK marked rows of ONE column octet (the candidates of a real frame gather in few
// columns: a grid split by column alone leaves most blocks idle).  Chunk c of the launch belongs to the column octet whose
// prefix of chunk counts holds it; a resident grid takes chunks blockIdx.x, + gridDim.x, ... and restages the weights only
// when the column octet changes.
#define FILL_CHUNK 64
// 512 threads = 64 items of 8 lanes per round: two such blocks give a SIMD four waves to cover the dependent chain's LDS reads
__global__ __launch_bounds__(512) void logit_fill_kernel(const ScreenArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    float *wl = (float *)lds;                                       // [9 * Cin][8]
    __shared__ int cbeg[SCREEN_MAX_OCT + 1];                        // first chunk of every column octet
    const int NO = a.Cout >> 3;
    if (threadIdx.x == 0) {
        int t = 0;
        for (int o = 0; o < NO; ++o) { cbeg[o] = t; t += (a.counts[o] + FILL_CHUNK - 1) / FILL_CHUNK; }
        cbeg[NO] = t;
    }
    __syncthreads();
    const int total = cbeg[NO];
    const int Cin = a.Cin, K = 9 * Cin;
    const int c = threadIdx.x & 7;
    int staged = -1, o = 0;
    float bias = 0.0f;
    for (int ch = blockIdx.x; ch < total; ch += gridDim.x) {        // (block-uniform)
        while (cbeg[o + 1] <= ch) ++o;
        if (o != staged) {
            __syncthreads();                                        // (every lane is done with the previous column's weights)
            for (int idx = threadIdx.x; idx < K * 8; idx += 512) {
                const int k = idx % Cin, cc = (idx / Cin) & 7, tap = idx / (Cin * 8);
                wl[(tap * Cin + k) * 8 + cc] = a.wt[((long long)tap * a.CoutPad + o * 8 + cc) * Cin + k];
            }
            __syncthreads();
            staged = o;
            bias = a.bias[o * 8 + c];
        }
        const int n = a.counts[o];
        const int *list = a.lists + (long long)o * a.rows_total;
        const int first = (ch - cbeg[o]) * FILL_CHUNK;
        const int last = first + FILL_CHUNK < n ? first + FILL_CHUNK : n;
        for (int it = first + (threadIdx.x >> 3); it < last; it += 64) {
            const int r = list[it];
            const ScreenLevel L = screen_level_of_row(a, r);
            const int m = r - L.row_begin;
            const int b = m / L.P, p = m - b * L.P;
            const int oy = p / L.W, ox = p - oy * L.W;
            const float *xb = a.x + L.in_off + (long long)b * L.P * Cin;
            float acc = 0.0f;
            for (int tap = 0; tap < 9; ++tap) {
                const int ky = tap / 3, kx = tap - 3 * ky;
                const int iy = oy + ky - 1, ix = ox + kx - 1;
                const bool ok = ((unsigned)iy < (unsigned)L.H) & ((unsigned)ix < (unsigned)L.W);
                const float *xp = xb + (long long)(ok ? iy * L.W + ix : 0) * Cin;
                const float *wp = wl + tap * Cin * 8 + c;
#pragma unroll 4
                for (int k8 = 0; k8 < Cin; k8 += 8) {
                    v4f v0 = *(const v4f *)(xp + k8), v1 = *(const v4f *)(xp + k8 + 4);
                    if (!ok) { v0 = v4f{0.f, 0.f, 0.f, 0.f}; v1 = v0; }       // a padded tap: zero operands (the load itself stays in range)
                    // logical channels 0..7 of the octet sit at physical 0,4,1,5,2,6,3,7 (ssd_internal.h)
                    acc = __builtin_fmaf(v0[0], wp[(k8 + 0) * 8], acc);
                    acc = __builtin_fmaf(v1[0], wp[(k8 + 4) * 8], acc);
                    acc = __builtin_fmaf(v0[1], wp[(k8 + 1) * 8], acc);
                    acc = __builtin_fmaf(v1[1], wp[(k8 + 5) * 8], acc);
                    acc = __builtin_fmaf(v0[2], wp[(k8 + 2) * 8], acc);
                    acc = __builtin_fmaf(v1[2], wp[(k8 + 6) * 8], acc);
                    acc = __builtin_fmaf(v0[3], wp[(k8 + 3) * 8], acc);
                    acc = __builtin_fmaf(v1[3], wp[(k8 + 7) * 8], acc);
                }
            }
            a.logits[L.out_off + (long long)b * a.out_bstride + (long long)p * a.out_rstride + o * 8 + c] = acc + bias;
        }
    }
}

// Host-side checks of everything the kernels assume (shapes, 32-bit offsets, capacities)
static bool screen_args_ok(const ScreenArgs &a)
{
    if (!a.x || !a.x16 || !a.w16 || !a.wt || !a.bias || !a.cst || !a.logits || !a.bits || !a.counts || !a.lists) return false;
    if (a.Cin % 64 != 0 || a.Cin < 64 || a.Cout % 8 != 0 || a.Cout < 8 || a.Cout > 8 * SCREEN_MAX_OCT || a.Cout > a.CoutPad) return false;
    if (a.NT != (a.Cout + 127) / 128 || a.nlevels < 1 || a.nlevels > SCREEN_MAX_LEVELS) return false;
    // (the signed plane's 32-bit byte offsets; two fill blocks per CU, each with its column octet's weights in LDS)
    if ((long long)9 * a.NT * 128 * a.Cin * 2 >= (1LL << 31) || (long long)9 * a.Cin * 8 * 4 > 160 * 1024 / 2) return false;
    if (a.out_rstride != a.Cout || a.out_bstride <= 0 || (a.out_bstride & 7) || (long long)a.B * a.out_bstride * 4 >= (1LL << 31)) return false;
    long long rows = 0, tiles = 0, outs = 0;
    for (int i = 0; i < a.nlevels; ++i) {
        const ScreenLevel &L = a.lv[i];
        if (L.P != L.H * L.W || L.M != a.B * L.P || L.P < 1 || L.row_begin != rows || L.tile_begin != tiles) return false;
        if ((long long)a.B * L.P * a.Cin * 4 >= (1LL << 31) || L.out_off != outs || (L.out_off & 7)) return false;
        rows += L.M;
        tiles += (L.M + 255) / 256;
        outs += (long long)L.P * a.out_rstride;
    }
    return rows == a.rows_total && tiles == a.tiles_m && outs == a.out_bstride && tiles * a.NT <= 0x7fffffffLL;
}

hipError_t launch_logit_convert(const ScreenArgs &a, hipStream_t s)
{
    if (!screen_args_ok(a) || a.x_elems <= 0 || (a.x_elems & 7)) return hipErrorInvalidValue;
    const long long n8 = a.x_elems / 8;
    const long long nblk = (n8 + 255) / 256;
    hipLaunchKernelGGL(logit_convert_kernel, dim3((unsigned)(nblk < 8192 ? nblk : 8192)), dim3(256), 0, s, a.x, a.x16, n8);
    return hipGetLastError();
}

hipError_t launch_logit_screen(const ScreenArgs &a, hipStream_t s)
{
    if (!screen_args_ok(a)) return hipErrorInvalidValue;
    constexpr int lds_bytes = SCREEN_STAGES * SCREEN_STAGE_BYTES;       // 144 KB (the epilogue's 64 KB of sums lie in it)
    static std::atomic<unsigned> attr_done{0};
    hipError_t e = ssd_allow_lds((const void *)logit_screen_kernel, lds_bytes, attr_done);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(logit_screen_kernel, dim3((unsigned)(a.tiles_m * a.NT)), dim3(256), lds_bytes, s, a);
    return hipGetLastError();
}

hipError_t launch_logit_fill(const ScreenArgs &a, hipStream_t s)
{
    if (!screen_args_ok(a)) return hipErrorInvalidValue;
    const long long nwords = ((long long)a.B * a.out_bstride / 8 + 31) / 32;
    const long long cblk = (nwords + 255) / 256;
    hipLaunchKernelGGL(logit_compact_kernel, dim3((unsigned)(cblk < 4096 ? cblk : 4096)), dim3(256), 0, s, a, nwords);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int lds_bytes = 9 * a.Cin * 8 * 4;
    static std::atomic<unsigned> attr_done{0};
    e = ssd_allow_lds((const void *)logit_fill_kernel, lds_bytes, attr_done);
    if (e != hipSuccess) return e;
    // a resident grid: two blocks per CU (the weights of a column octet are 72 KB of a CU's 160 KB), never more blocks than chunks
    // can exist
    long long maxchunks = ((long long)a.rows_total + FILL_CHUNK - 1) / FILL_CHUNK * (a.Cout / 8);
    static std::atomic<int> cu_count{0};                            // (asked once: the launch path calls no other HIP API)
    int cus = cu_count.load(std::memory_order_relaxed);
    if (cus <= 0) {
        int dev = 0;
        cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (cus <= 0) cus = 256;
        cu_count.store(cus, std::memory_order_relaxed);
    }
    const long long grid = maxchunks < 2LL * cus ? maxchunks : 2LL * cus;
    hipLaunchKernelGGL(logit_fill_kernel, dim3((unsigned)grid), dim3(512), lds_bytes, s, a);
    return hipGetLastError();
}
