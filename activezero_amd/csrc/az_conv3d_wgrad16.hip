// Weight gradient of the stride-1 3x3x3 layers (bf16x6): the V0 32 -> 32 layers and, as 2 x 2 tiles of 32 x 32 channels in
// the grid, the 64 -> 64 layers of the hourglasses (0.94 -> 0.84 ms at 1/8 resolution, 0.44 -> 0.50 of the roofline),
// rebuilt the way az_conv3d_roll.hip rebuilt the
// forward / input-gradient kernel (psmnet_3.py:87-117 dres0..dres4 / classif convs; G = dW[co][ci][27]):
//
//   G[m][n][kd,kh,kw] = sum over positions (b, d, h, w) of  coarse[b,d,h,w][m] * fine[b, d-1+kd, h-1+kh, w-1+kw][n]
//
// az_conv3d_wgrad.hip gives a wave ONE kd (nine 32x32 accumulators = 144 registers): the coarse row is fetched, split
// into its bf16 triplet and written to LDS by three waves, every fine row by three waves too, and that staging sits
// between two barriers of a one-wave workgroup (20-30 % of the kernel, profiles/r02_clock_pipe_ablation.md section 7).
// Here, on the 16x16x32 bf16 MFMA:
//   * a wave owns a 16 x 16 block (half of the coarse channels x half of the fine channels) of ALL 27 taps: 27 x 4 = 108
//     accumulator registers; four waves = one workgroup cover 32 x 32 and share every staged byte;
//   * K = 32 positions per MFMA = two adjacent coarse rows x 16 positions (240 = 15 x 16: no padded positions); a step
//     is 27 taps x 6 MFMAs per wave and needs, staged, 2 coarse rows and the 4-row window of three fine planes, of which
//     only 2 coarse + 3 x 2 fine rows are new: 140 positions per 162 MFMAs x 4 waves (was 34 per 54 MFMAs x 1 wave);
//   * the coarse pair is double-buffered, each fine plane keeps a ring of six rows: the next step's rows are split and
//     written while this step is multiplied (one barrier per step); loads, validity (zero padding in h / w / d) and
//     therefore vmcnt bookkeeping go through buffer instructions with out-of-range offsets: a step is one basic block;
//   * workgroups are persistent: each walks a list of (batch, coarse depth, 16-position chunk) columns and flushes its
//     27 x 32 x 32 block once, with float atomics, into the tap-major workspace of az_conv3d_wgrad.hip.
// Arithmetic per K block: the six-MFMA chain of az_wgrad_common.h (smallest terms first, fp32 accumulate).
//
// Measured (B=4, V0; profiles/r03_roll_kernel_notes.md section 5): 1.65-1.74 ms against 1.76-1.80 ms for the one-kd-per-
// wave kernel on the same boxes -- staging is now a third per MFMA and hidden, LDS bank conflicts are gone (46 % of the
// LDS cycles before the row-half swap), but a 16x16 block per tap gives every fine fragment exactly ONE use: 168
// transposing reads per 162 MFMAs, twice the LDS instructions per matrix cycle of the 32x32x16 form, and the kernel is
// bound by instruction issue (4.1 instructions per 16-cycle MFMA; +4 VALU per tap cost +15 %, fragments two taps ahead
// with recomputed addresses +13 %).
#include <stdlib.h>

#include "az_wgrad_common.h"
#include "az_options.h"

#define W16_POS 16                       // positions of a coarse row per step
#define W16_FW (W16_POS + 2)             // fine positions per staged row
#define W16_ROWB AZ_W16_ROWB             // bytes of one (position, 32 channels) bf16 row
#define W16_CBUF (3 * 32 * W16_ROWB)     // one coarse buffer: [part][k = 2 rows x 16][32 ch]      6 144 B
#define W16_FROW (3 * W16_FW * W16_ROWB) // one fine row: [part][18 positions][32 ch]              3 456 B
#define W16_RING 6
#define W16_LDS (2 * W16_CBUF + 3 * W16_RING * W16_FROW)  // 74 496 B
#define W16_NPOS (2 * W16_POS + 3 * 2 * W16_FW)           // positions staged per step: 140
#define W16_NQ (W16_NPOS * 8)                              // float4 pieces: 1 120
#define W16_NLD ((W16_NQ + 255) / 256)                     // 5 per thread
#define W16_OOB 0xffffff00u

struct Wg16Args {
    const float *coarse, *fine;
    float *ws;  // [27][CM][CN]
    int B, D, H, W;
    int CM, CN;  // channels of coarse / fine (32 or 64 each): one workgroup owns ONE 32 x 32 (m, n) tile
    int nwchunk;
    long long ncols;  // B * D * nwchunk columns of work
    int wgs;          // persistent workgroups per tile
    int xcd;          // XCD-chunked column order
    const float *coarse_amax, *fine_amax;  // f16x3 (AR = 1): device scalars max |coarse|, max |fine|
};

// AR: 0 = bf16x6 (three bf16 parts, six MFMAs per tap), 1 = f16x3 (two scaled fp16 parts, three MFMAs; az_roll_common.h).
// The LDS images keep their three-part strides either way (the third part is unused with AR = 1).
// PSM (AR = 1): bit 0 = the coarse operand, bit 1 = the fine operand is a pre-split tensor (az_roll_common.h).
template <int AR, int PSM = 0>
__global__ void __launch_bounds__(256, 2)
conv3d_wgrad_r16_kernel(const Wg16Args a) {
    constexpr int NP = AR ? 2 : 3;
    __shared__ __attribute__((aligned(16))) unsigned char lds[W16_LDS + 64];  // + a sink for the lanes of a partial piece
    unsigned char *const cbuf = lds;                  // [2][W16_CBUF]
    unsigned char *const fring = lds + 2 * W16_CBUF;  // [plane kd][slot][W16_FROW]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mi = wv >> 1, ni = wv & 1;
    // 64-channel operands: 2 x 2 (or 2 x 1 / 1 x 2) tiles in the grid; the workgroups of tile t are blockIdx.x in [t wgs, (t + 1) wgs)
    const int ntn = a.CN >> 5;
    // workgroups b and b + 8 share an XCD (and its L2): each XCD gets a contiguous run of the column list -- neighbouring depths
    // of one chunk, which read the same fine planes -- instead of every eighth column (AZ_WGRAD_R16_XCD=0: the linear order)
    const int tile = blockIdx.x / a.wgs, wgl = blockIdx.x - tile * a.wgs;
    const int wg0 = (a.xcd && !(a.wgs & 7)) ? az_xcd_map(wgl, a.wgs) : wgl;
    const int m0 = (tile / ntn) * 32, n0 = (tile % ntn) * 32;

    f32x4 acc[27];
#pragma unroll
    for (int t = 0; t < 27; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float c_scale = 1.f, f_scale = 1.f, o_scale = 1.f;
    if (AR) az_f16_scales(a.coarse_amax, a.fine_amax, c_scale, o_scale, &f_scale);

    // transposing-read geometry and the row-half swap against bank conflicts: az_w16_lanes (az_launch_math.h), written out
    // (called as a function it moves this kernel's registers: <1, .> 244 -> 243, <0, 0> 11 -> 7 spilled)
    const int oct = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
    const unsigned a_lane = (unsigned)(8 * oct + tq) * W16_ROWB + (((unsigned)(16 * mi + 4 * tp) * 2) ^ ((unsigned)(oct & 1) << 5));
    // fine: the offsets inside one staged row, per kw; the row-in-window part is added per step (ring slots)
    const int rp = oct >> 1;
    unsigned b_off[3][2];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            const unsigned rowi = (unsigned)(8 * (oct & 1) + tq + kw + 4 * h2);
            b_off[kw][h2] = rowi * W16_ROWB + (((unsigned)(16 * ni + 4 * tp) * 2) ^ (((rowi >> 3) & 1u) << 5));
        }

    const unsigned vb_c = (unsigned)a.CM * 4u, vb_f = (unsigned)a.CN * 4u;  // bytes per voxel
    const unsigned plane_c = (unsigned)a.H * a.W * vb_c, plane_f = (unsigned)a.H * a.W * vb_f;
    for (long long col = wg0; col < a.ncols; col += a.wgs) {
        // column -> (w chunk, coarse depth, batch); consecutive columns = consecutive depths of one chunk: the
        // workgroups resident together read neighbouring planes of the same rows (one L2 serves the three kd)
        long long r_ = col;
        const int cd = (int)(r_ % a.D); r_ /= a.D;
        const int wc = (int)(r_ % a.nwchunk);
        const int b = (int)(r_ / a.nwchunk);
        const int cw0 = wc * W16_POS;
        const unsigned vol_c = (unsigned)a.D * plane_c, vol_f = (unsigned)a.D * plane_f;
        const auto rs_c = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.coarse) + (size_t)b * (vol_c / 4) + m0, 0, vol_c, 0x00020000);
        const auto rs_f = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.fine) + (size_t)b * (vol_f / 4) + n0, 0, vol_f, 0x00020000);

        // ---- staging set of step s: coarse rows 2s, 2s+1 (buffer s & 1); fine rows 2s-1+{2,3}... see below ----------
        // piece q = tid + 256 it of a set:  q < 256: coarse (row pair, 16 positions, 8 float4 per position);
        // q >= 256: fine, plane kd = (q - 256) / 288, new row j = .. / 144, position .. / 8  (18 x 8 = 144 per row)
        u32x4 pre[W16_NLD];
        auto issue = [&](int crow0, bool with_coarse, int frow0) {  // coarse rows crow0, crow0+1; fine rows frow0, frow0+1
#pragma unroll
            for (int it = 0; it < W16_NLD; ++it) {
                const int q = tid + 256 * it;
                unsigned off = W16_OOB;
                if (it == 0) {  // q < 256: coarse
                    const int k = q >> 3, row = crow0 + (k >> 4), cw = cw0 + (k & 15);
                    if (with_coarse && row < a.H && cw < a.W)
                        off = (unsigned)cd * plane_c + (unsigned)(row * a.W + cw) * vb_c + (unsigned)(q & 7) * 16u;
                    pre[it] = __builtin_amdgcn_raw_buffer_load_b128(rs_c, off, 0, 0);
                } else {
                    const int f = q - 256;
                    const int kd = f / 288, g = f - kd * 288;
                    const int j = g / 144, pp = (g - j * 144) >> 3;
                    const int fd = cd - 1 + kd, fr = frow0 + j, fw = cw0 - 1 + pp;
                    if (q < W16_NQ && (unsigned)fd < (unsigned)a.D && (unsigned)fr < (unsigned)a.H && (unsigned)fw < (unsigned)a.W)
                        off = (unsigned)fd * plane_f + (unsigned)(fr * a.W + fw) * vb_f + (unsigned)(q & 7) * 16u;
                    pre[it] = __builtin_amdgcn_raw_buffer_load_b128(rs_f, off, 0, 0);
                }
            }
        };
        auto commit_piece = [&](int it, int cbuf_idx, int frow0) {
            const int q = tid + 256 * it;
            uint2 hi, mid, lo;
            if (it == 0) az_wgrad_split<AR, (PSM & 1) != 0>(pre[it], c_scale, hi, mid, lo);
            else az_wgrad_split<AR, (PSM & 2) != 0>(pre[it], f_scale, hi, mid, lo);
            unsigned char *dst;
            unsigned part_stride;
            if (it == 0) {
                dst = cbuf + cbuf_idx * W16_CBUF + az_w16_piece_off(q >> 3, q);
                part_stride = 32 * W16_ROWB;
            } else {
                const int f = q - 256;
                const int kd = f / 288, g = f - kd * 288;
                const int j = g / 144, pp = (g - j * 144) >> 3;
                const int slot = (frow0 + j + W16_RING) % W16_RING;
                dst = fring + (kd * W16_RING + slot) * W16_FROW + az_w16_piece_off(pp, q);
                part_stride = W16_FW * W16_ROWB;
            }
            if (q >= W16_NQ) { dst = lds + W16_LDS + (tid & 7) * 8; part_stride = 0; }  // (no branch: a step stays one block)
            az_wgrad_store_parts<AR>(dst, part_stride, hi, mid, lo);
        };

        // ---- prologue: the window of step 0 (fine rows -1 .. 2, coarse rows 0, 1), then the request for step 1 -------
        __syncthreads();  // the previous column's last step no longer reads
        issue(0, false, -1);
#pragma unroll
        for (int it = 0; it < W16_NLD; ++it) commit_piece(it, 0, -1);
        issue(0, true, 1);
#pragma unroll
        for (int it = 0; it < W16_NLD; ++it) commit_piece(it, 0, 1);
        issue(2, true, 3);
        __syncthreads();

        const int nsteps = (a.H + 1) / 2;
        for (int s = 0; s < nsteps; ++s) {
            const int ch = 2 * s;
            const unsigned char *ca = cbuf + (s & 1) * W16_CBUF + a_lane;
            // ring slots of fine rows ch-1 .. ch+2 (wave-uniform), then this lane's (rows rp + kh)
            int slot[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) slot[r] = (ch - 1 + r + W16_RING) % W16_RING;
            unsigned fb[3];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) fb[kh] = (unsigned)(rp ? slot[kh + 1] : slot[kh]) * W16_FROW;

            az_bf16x8 af[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) af[p] = __builtin_bit_cast(az_bf16x8, az_tr16_frag(ca + p * 32 * W16_ROWB, ca + p * 32 * W16_ROWB + 4 * W16_ROWB));
            az_bf16x8 bf[2][NP];
            auto load_b = [&](az_bf16x8 (&bq)[NP], int t) {
                const int kd = t / 9, kh = (t % 9) / 3, kw = t % 3;
                const unsigned char *fp = fring + kd * (W16_RING * W16_FROW) + fb[kh];
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    bq[p] = __builtin_bit_cast(az_bf16x8, az_tr16_frag(fp + b_off[kw][0] + p * W16_FW * W16_ROWB, fp + b_off[kw][1] + p * W16_FW * W16_ROWB));
            };
            load_b(bf[0], 0);
#pragma unroll
            for (int t = 0; t < 27; ++t) {
                __builtin_amdgcn_sched_barrier(0);
                if (t + 1 < 27) load_b(bf[(t + 1) & 1], t + 1);
                __builtin_amdgcn_sched_barrier(0);
                az_wgrad_chain<AR>(acc[t], af, bf[t & 1]);
                // the set of step s+1 (requested a step ago): one piece after each of the taps 1, 3, 5, 7, 9; then the
                // request for step s+2 (17 taps + the next step's first ones to land)
                if (t >= 1 && t <= 9 && (t & 1)) {
                    __builtin_amdgcn_sched_barrier(0);
                    commit_piece((t - 1) / 2, (s + 1) & 1, ch + 3);
                }
                if (t == 10) {
                    __builtin_amdgcn_sched_barrier(0);
                    issue(ch + 4, true, ch + 5);
                }
            }
            __syncthreads();  // next step's rows written by all four waves; this step's no longer read
        }
    }
    // D[i][j]: i = coarse channel 16 mi + 4 (lane >> 4) + r, j = fine channel 16 ni + (lane & 15): az_wgrad_flush16 written out
    // (called as a function it moves this kernel's registers as the lane geometry above does)
#pragma unroll
    for (int t = 0; t < 27; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * mi + 4 * (lane >> 4) + r;
            atomicAdd(&a.ws[((size_t)t * a.CM + m) * a.CN + n0 + 16 * ni + (lane & 15)], AR ? acc[t][r] * o_scale : acc[t][r]);
        }
}

// Round 5 built this kernel a second time with TAPS, not channel blocks, split over the four waves ("wide tile": a wave owns
// the whole 32 x 32 channel tile of seven taps on v_mfma_f32_32x32x16_f16; per wave and step 64 transposing LDS reads for 42
// MFMAs of 32 cycles, against 114 reads for 81 MFMAs of 16 cycles here).  MEASURED (profiles/r05l_wgrad_wide_vs_narrow.md;
// DESIGN.md 4a): SQ_WAIT_INST_LDS 1.6e8 -> 3.9e7, SQ_LDS_IDX_ACTIVE 2.3e8 -> 1.3e8, bank conflicts 1.4e7 -> 0, wave cycles
// 9.2e8 -> 8.0e8 (-13 %) -- and the SAME time, 1.12 against 1.11 ms alone, 85.6 against 85.4 ms per step: the chip gives the
// saved cycles back as clock (the 32x32x16 shape holds a lower clock than 16x16x32 at equal flops).  At this matrix rate the
// V0 weight gradient is bound by what the part sustains under fp16 MFMA load, not by its LDS traffic.  That kernel is no
// longer in the tree (DESIGN.md section 4 names the last tree that has it).


// persistent workgroups: at most 512 resident (2 per CU); the count that balances the columns best
int az_conv3d_wgrad_r16_launch(float *ws, const float *coarse, const float *fine, int B, int cm, int cn, int D, int H, int W, hipStream_t s,
                               const float *coarse_amax, const float *fine_amax, int split_mask) {
    if (!((cm == 32 || cm == 64) && (cn == 32 || cn == 64))) return AZ_EUNSUPPORTED;
    Wg16Args a{};
    a.coarse = coarse; a.fine = fine; a.ws = ws; a.coarse_amax = coarse_amax; a.fine_amax = fine_amax;
    a.B = B; a.D = D; a.H = H; a.W = W; a.CM = cm; a.CN = cn;
    const int ntiles = (cm / 32) * (cn / 32);
    const int slots = 512 / ntiles;  // resident workgroups per tile (two per CU)
    a.nwchunk = (W + W16_POS - 1) / W16_POS;
    a.ncols = (long long)B * D * a.nwchunk;
    if (!az_fits_buffer_offset((long long)D * H * W * (cm > cn ? cm : cn) * 4)) return AZ_EUNSUPPORTED;  // one batch element through a 32-bit offset
    const int best = az_wgrad16_workgroups(a.ncols, slots, ntiles, az_options().wgrad_r16_wgs);
    a.wgs = best;
    a.xcd = az_options().wgrad_r16_xcd;
    const dim3 grid((unsigned)(a.wgs * ntiles));
    if (!(coarse_amax && fine_amax)) {
        if (split_mask) return AZ_EINVAL;
        hipLaunchKernelGGL(conv3d_wgrad_r16_kernel<0>, grid, dim3(256), 0, s, a);
    } else if (!az_wgrad_split_dispatch<3>(split_mask, [&](auto psm) {
                   hipLaunchKernelGGL((conv3d_wgrad_r16_kernel<1, decltype(psm)::value>), grid, dim3(256), 0, s, a);
               }))
        return AZ_EINVAL;
    return az_launch_status();
}
