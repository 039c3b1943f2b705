// Host-side (and host/device) launch arithmetic of the tiled kernels, free of HIP types so that the SAME functions the
// launches use are also compiled with g++ -fsanitize=address,undefined and swept over shapes on the CPU
// (tests/host/launch_math_test.cpp, tests/test_launch_math_cpu.py; SURVEY.md 5.2: "a host check of the launch
// arithmetic").  Device code includes it too: AZ_HD marks what a kernel calls.
#pragma once
#if defined(__HIPCC__)
#define AZ_HD __host__ __device__ __forceinline__
#else
#define AZ_HD inline
#endif

// Workgroup -> work-item map shared by every tiled kernel: blocks b and b + 8 share an XCD (and its L2), so each XCD gets
// ONE contiguous chunk of the linear order.  A bijection of [0, nblk) for every nblk >= 1.
AZ_HD int az_xcd_map(int bid, int nblk) {
    const int xcd = bid & 7, q8 = nblk >> 3, r8 = nblk & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// Block -> tile map of the gather kernels (az_conv3d.hip, az_conv3d_m128.hip, az_conv3d_t2.hip): position `lin` of the linear
// tile order (map_mode 0: the block id; >= 1: az_xcd_map of it, so that an XCD walks a contiguous chunk) -> patch column tix,
// tile row tiy < rows_y, depth index td < Dt, batch entry b.  map_mode < 2: the plain mixed radix, x fastest, then rows,
// depth, batch.  map_mode >= 2, banded: x fastest, then the band_rows tile rows of a band, then the depth index, then the
// band (the last one may have fewer rows) -- the three output planes that read one input plane, and the row halos inside a
// band, are processed back to back and hit in L2.  A bijection of [0, B * Dt * rows_y * tiles_x) onto the tiles either way.
AZ_HD void az_conv_tile_decode(int lin, int map_mode, int band_rows, int tiles_x, int rows_y, int Dt, int &tix, int &tiy,
                               int &td, int &b) {
    tix = lin % tiles_x; lin /= tiles_x;
    if (map_mode >= 2) {
        const int per_b = Dt * rows_y;
        b = lin / per_b;
        int l = lin - b * per_b;
        const int full = (rows_y / band_rows) * band_rows * Dt;  // blocks in the complete bands
        int band, rows;
        if (l < full) { band = l / (band_rows * Dt); l -= band * band_rows * Dt; rows = band_rows; }
        else { band = rows_y / band_rows; l -= full; rows = rows_y - band * band_rows; }
        td = l / rows;
        tiy = band * band_rows + (l - td * rows);
    } else {
        tiy = lin % rows_y; lin /= rows_y;
        td = lin % Dt;
        b = lin / Dt;
    }
}

// The 24-dword slab image of az_conv3d_m128.hip, az_conv3d_t2.hip and az_conv2d.hip: a voxel is up to three 8-dword parts
// (16 channels of 16-bit values each) and a row is `pitch` voxels (== 4 mod 8); the two 16-byte halves of a part are swapped
// on odd rows, which makes the ds_read_b128 of an A fragment conflict-free without padding (az_conv3d_m128.hip).
// Writing: dword offset of the 8-byte piece j (channels 4j .. 4j + 3 of the chunk) of part 0 of voxel (sy, sx); part p: + 8p.
#define AZ_S24_VS 24
AZ_HD int az_s24_write_off(int sy, int sx, int j, int pitch) {
    return (sy * pitch + sx) * AZ_S24_VS + ((j >> 1) ^ (sy & 1)) * 4 + (j & 1) * 2;
}
// Reading: the 16 bytes = channels 8 half .. 8 half + 7 of part 0 that fragment lane (voxel (rty, rtx) of its 4x8 tile, K
// half `half`) takes from the voxel (dy, dx) further on, dy of the given parity; the read adds (dy * pitch + dx) * AZ_S24_VS.
AZ_HD int az_s24_read_base(int rty, int rtx, int half, int parity, int pitch) {
    return (rty * pitch + rtx) * AZ_S24_VS + (half ^ ((rty + parity) & 1)) * 4;
}

// az_conv3d_roll.hip: depth segments of a launch -- one round of workgroups over the chip's 512 slots (256 CUs x 2) if the
// patches allow it, otherwise the split that minimises rounds x (planes walked per workgroup).  patches = B * 8-row patch
// rows * patch columns; forced > 0: that segment length (AZ_ROLL_SEGLEN).  Postconditions: nseg * seg_len >= Do,
// (nseg - 1) * seg_len < Do, 1 <= seg_len <= Do.
inline void az_roll_segments(long long patches, int Do, int forced, int &nseg, int &seg_len) {
    if (forced > 0) {
        seg_len = forced < Do ? forced : Do;
        nseg = (Do + seg_len - 1) / seg_len;
        return;
    }
    long long best = -1;
    nseg = 1; seg_len = Do;
    for (int n = 1; n <= Do; ++n) {
        const int len = (Do + n - 1) / n;
        const int nn = (Do + len - 1) / len;
        if (nn != n) continue;
        const long long rounds = (patches * n + 511) / 512;
        const long long cost = rounds * (len + 2) * 3 + 2;  // +: fixed cost per workgroup
        if (best < 0 || cost < best) { best = cost; nseg = n; seg_len = len; }
    }
}

// az_conv3d_t2roll.hip: coarse-depth segments of a launch with ONE workgroup per CU (256 slots); a workgroup runs seg_len full
// stages and a closing one of nine of the 27 taps.  Postconditions as az_roll_segments.
inline void az_t2roll_segments(long long patches, int Di, int &nseg, int &seg_len) {
    long long best = -1;
    nseg = 1; seg_len = Di;
    for (int n = 1; n <= Di; ++n) {
        const int len = (Di + n - 1) / n;
        if ((Di + len - 1) / len != n) continue;
        const long long rounds = (patches * n + 255) / 256;
        const long long cost = rounds * (len * 4 + 2) + 1;
        if (best < 0 || cost < best) { best = cost; nseg = n; seg_len = len; }
    }
}

// az_conv3d_s2roll.hip: coarse-depth segments of a launch with two workgroups per CU (512 slots); a workgroup of a segment
// of len output planes stages 2 len + 1 fine planes and multiplies 27 len tap positions; a staged plane is priced at four
// tap positions (measured at B = 4, V0 -> V1, 288 patches: 0.34 ms for len 4 .. 6, 0.36 at 3, 0.38 at 1 and 12, 0.46 at 24).  forced > 0: that segment length (AZ_S2ROLL_SEGLEN).  Postconditions as az_roll_segments.
inline void az_s2roll_segments(long long patches, int Do, int forced, int &nseg, int &seg_len, int slots = 512) {
    if (forced > 0) {
        seg_len = forced < Do ? forced : Do;
        nseg = (Do + seg_len - 1) / seg_len;
        return;
    }
    long long best = -1;
    nseg = 1; seg_len = Do;
    for (int n = 1; n <= Do; ++n) {
        const int len = (Do + n - 1) / n;
        if ((Do + len - 1) / len != n) continue;
        const long long rounds = (patches * n + slots - 1) / slots;
        const long long cost = rounds * (27LL * len + 4 * (2 * len + 1) + 4);
        if (best < 0 || cost < best) { best = cost; nseg = n; seg_len = len; }
    }
}

// az_conv2d_roll.hip: image segments per statistic group (patches = groups * patch rows * patch columns; N images)
inline void az_c2r_segments(long long patches, int N, int &nseg, int &seg_len) {
    long long best = -1;
    nseg = 1; seg_len = N;
    for (int n = 1; n <= N; ++n) {
        const int len = (N + n - 1) / n;
        if ((N + len - 1) / len != n) continue;
        const long long rounds = (patches * n + 511) / 512;
        const long long cost = rounds * (len * 3 + 2);  // stages per workgroup + its fixed cost
        if (best < 0 || cost < best) { best = cost; nseg = n; seg_len = len; }
    }
}

// az_conv3d_c1.hip, forward: depth segment per workgroup.  Every segment stages 2 halo planes, and the grid should fill a
// whole number of residency rounds (3 workgroups per CU x 256 CUs by registers): the dseg = ceil(D / n) that minimises
// rounds x (dseg + 2), the longest one among equals.  patches = B * 8-row patch rows * 16-voxel patch columns.
// Postconditions: 1 <= dseg <= D; the nseg = ceil(D / dseg) segments have (nseg - 1) * dseg < D.
#define AZ_C1_FWD_SLOTS 768
inline long long az_c1_fwd_cost(long long patches, int D, int dseg) {
    const long long blocks = patches * ((D + dseg - 1) / dseg);
    return ((blocks + AZ_C1_FWD_SLOTS - 1) / AZ_C1_FWD_SLOTS) * (dseg + 2);
}
inline int az_c1_fwd_dseg(long long patches, int D) {
    int best = 1;
    long long best_cost = -1;
    for (int nseg = 1; nseg <= D; ++nseg) {
        const int dseg = (D + nseg - 1) / nseg;
        const long long cost = az_c1_fwd_cost(patches, D, dseg);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = dseg; }
    }
    return best;
}
// az_conv3d_c1.hip, weight gradient: workgroup g of `grid` walks the (batch, plane, 8 x 32 tile) items g, g + grid, ...
#define AZ_C1_WGRAD_MAX_GRID 2048
inline long long az_c1_wgrad_tiles(int B, int D, int H, int W) {
    return (long long)B * D * ((H + 7) / 8) * ((W + 31) / 32);
}
inline int az_c1_wgrad_grid(long long ntiles) {
    return (int)(ntiles < AZ_C1_WGRAD_MAX_GRID ? ntiles : AZ_C1_WGRAD_MAX_GRID);
}

// linear index -> (patch column, 8-row patch row, depth segment, batch) of az_conv3d_roll.hip
AZ_HD void az_roll_decode(int lin, int tiles_x, int tyb, int nseg, int &tix, int &tiy, int &seg, int &b) {
    tix = lin % tiles_x; lin /= tiles_x;
    tiy = lin % tyb; lin /= tyb;
    seg = lin % nseg;
    b = lin / nseg;
}

// Slab staging of the rolling kernels: 10 x 18 voxels x 8 sixteen-byte pieces, 256 threads, piece q = tid + 256 it; thread
// tid's it-th piece is voxel (tid >> 3) + 32 it.  The kernels step (sy, sx) incrementally (32 voxels = one 18-voxel row +
// 14); this is the closed form the CPU test compares the stepping against.
#define AZ_R_SY 10
#define AZ_R_SX 18
#define AZ_R_NQ (AZ_R_SY * AZ_R_SX * 8)
AZ_HD bool az_roll_piece(int tid, int it, int &sy, int &sx) {
    const int vox = (tid >> 3) + 32 * it;
    sy = vox / AZ_R_SX;
    sx = vox - sy * AZ_R_SX;
    return tid + 256 * it < AZ_R_NQ;
}

// az_conv3d_wgrad16.hip: persistent workgroups per (m, n) tile -- at most `slots` resident (two per CU over the tiles), the
// count that balances the columns best; cap > 0: AZ_WGRAD_R16_WGS.  1 <= result <= max(1, min(slots, ncols)).
inline int az_wgrad16_workgroups(long long ncols, int slots, int ntiles, int cap) {
    int best = 1;
    double best_score = -1.0;
    const int step = 8 / (ntiles > 2 ? 4 : ntiles);
    for (int w = slots; w >= slots / 4 && w >= 1; w -= step) {
        if (w > ncols) continue;
        const long long per = (ncols + w - 1) / w;
        const double score = (double)ncols / (double)(per * slots);  // useful fraction of the chip-time taken
        if (score > best_score + 1e-9) { best_score = score; best = w; }
    }
    if (ncols < slots / 4) best = (int)(ncols > 0 ? ncols : 1);
    if (cap > 0 && cap < best) best = cap;
    return best;
}

// C layout of the two MFMA shapes the weight-gradient kernels flush (az_wgrad_common.h) and the gather kernels store
// (az_gather_common.h): register `reg` of lane `lane` holds element (row, col) of the tile -- 32x32: 16 registers, 16x16: 4
// registers.  (_h: by the lane's half-wave lane >> 5, for kernels that keep it -- hipcc does not merge a second lane >> 5
// with theirs, and az_conv3d.hip then spills in 11 instantiations.)
AZ_HD int az_mfma32_c_row_h(int half, int reg) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }
AZ_HD int az_mfma32_c_row(int lane, int reg) { return az_mfma32_c_row_h(lane >> 5, reg); }
AZ_HD int az_mfma32_c_col(int lane) { return lane & 31; }
AZ_HD int az_mfma16_c_row(int lane, int reg) { return 4 * (lane >> 4) + reg; }
AZ_HD int az_mfma16_c_col(int lane) { return lane & 15; }

// The r16 weight-gradient kernels' LDS images: [k row][32 channels] of 16-bit values, 64-byte rows = 16 banks, so rows r and
// r + 8 fall on the same banks -- and the two octets of a 32-lane half of a transposing read address exactly such rows (a
// 2-way conflict on every read, measured: 46 % of the LDS cycles).  The two 32-byte channel halves of a row are therefore
// swapped on rows with bit 3 set: writes and reads XOR the in-row byte offset with az_w16_half_swap(row).
#define AZ_W16_ROWB 64
AZ_HD unsigned az_w16_half_swap(unsigned row) { return ((row >> 3) & 1u) << 5; }
// staging: byte offset of the 8-byte piece q & 7 (channels 4 (q & 7) ..) of row `row`; q: the float4 piece index of the staging loops
AZ_HD int az_w16_piece_off(int row, int q) { return row * AZ_W16_ROWB + (((q & 7) * 8) ^ (((row >> 3) & 1) << 5)); }
// reading: the address lane 4q + p of a 16-lane group supplies for rows row0 .. row0 + 3 of the channel block from ch0 (0 or
// 16): row row0 + q, channels ch0 + 4p ..
AZ_HD unsigned az_w16_read_off(int lane, unsigned row0, unsigned ch0) {
    const unsigned row = row0 + ((unsigned)(lane & 15) >> 2);
    return row * AZ_W16_ROWB + (((ch0 + 4 * (unsigned)(lane & 3)) * 2) ^ az_w16_half_swap(row));
}
// Lane geometry of a K = 32 step = two coarse rows x 16 positions: octet oct = lane >> 4 holds k rows 8 oct ..; of the fine
// window it reads row-of-the-pair rp = oct >> 1, positions 8 (oct & 1) .. shifted by the tap's kw (+ 4: the second half of a
// fragment).  a_ch0 / b_ch0: the wave's 16-channel block inside the coarse / fine 32-channel image.
struct AzW16Lanes { unsigned a_lane, b_off[3][2]; int rp; };
AZ_HD AzW16Lanes az_w16_lanes(int lane, unsigned a_ch0, unsigned b_ch0) {
    const unsigned oct = (unsigned)lane >> 4;
    AzW16Lanes g;
    g.a_lane = az_w16_read_off(lane, 8 * oct, a_ch0);
    g.rp = (int)(oct >> 1);
    for (int kw = 0; kw < 3; ++kw)
        for (int h2 = 0; h2 < 2; ++h2) g.b_off[kw][h2] = az_w16_read_off(lane, 8 * (oct & 1) + kw + 4 * h2, b_ch0);
    return g;
}

// az_conv2d_wgrad16.hip (3x3 d1 2-D weight gradient, 32 / 64 channels): a column of work = (image, 16-position chunk, row
// segment); `slots` = workgroups resident per (co, ci) tile (768 / ntiles at three per CU; 256 for the one-tile-per-workgroup
// 64 x 64 kernel).  Row segments have EVEN row counts (a step multiplies a pair of dy rows): of the up to 16 splits the one
// with the best (column balance) x (occupancy) x (rows per window prologue).  Postconditions: seg_rows even,
// nrseg * seg_rows >= H, (nrseg - 1) * seg_rows < H, ncols = B * ceil(W / 16) * nrseg, 1 <= wgs <= min(slots, ncols).
struct AzC2w16Plan { int seg_rows, nrseg, wgs; long long ncols; };
inline AzC2w16Plan az_c2w16_plan(int B, int H, int W, int slots) {
    const int nwchunk = (W + 15) / 16;
    AzC2w16Plan p{};
    p.nrseg = 1; p.wgs = 1;
    double best = -1.0;
    for (int nseg = 1; nseg <= 16; ++nseg) {
        int rows = (H + nseg - 1) / nseg;
        rows += rows & 1;
        const int segs = (H + rows - 1) / rows;
        const long long cols = (long long)B * nwchunk * segs;
        const int w = (int)(cols < slots ? cols : slots);
        const long long per = (cols + w - 1) / w;
        const double balance = (double)cols / (double)(per * w);
        const double occ = (double)w / (double)slots;
        const double amort = (double)rows / (double)(rows + 4);
        const double score = balance * (0.5 + 0.5 * occ) * amort;
        if (score > best) { best = score; p.nrseg = segs; p.wgs = w; p.seg_rows = rows; }
    }
    p.ncols = (long long)B * nwchunk * p.nrseg;
    return p;
}

// az_conv2d_wgrad.hip (the generic 2-D weight gradient, MT x NT waves per workgroup): static work lists -- block w of a
// (co, ci) combo takes items w, w + blocks_per_combo, ... of the nitems = B * ceil(W / 16) * nhseg (image, row segment,
// chunk) items; the kernel ends with its most loaded block, so (row segments, blocks per combo) are picked with the item count
// a near multiple of the block count while ncombo * blocks * MT * NT stays close to the resident waves.  ring_rows =
// DIL * (KH - 1) + 1 rows of x are staged before an item's first output row.  Postconditions: nhseg * hseg_rows >= H,
// (nhseg - 1) * hseg_rows < H, blocks_per_combo >= 8 and a multiple of 8 (blocks b and b + 8 share an XCD).
struct AzC2wPlan { int blocks_per_combo, hseg_rows, nhseg; long long nitems; };
inline AzC2wPlan az_c2w_plan(int B, int H, int W, int mt, int nt, int ncombo, int ring_rows) {
    const int nwchunk = (W + 15) / 16;
    const int slots = 256 * 8 / (mt * nt);  // resident workgroups at 2 waves/SIMD
    const int wq = (slots / ncombo) & ~7;
    const int wmax = wq > 8 ? wq : 8;
    const int wmin = wmax / 2 > 8 ? wmax / 2 : 8;
    const long long base_items = (long long)B * nwchunk;
    double best = -1.0;
    int best_w = 8, best_rows = H;
    for (int nseg = 1; nseg <= (H < 32 ? H : 32); ++nseg) {
        const int rows = (H + nseg - 1) / nseg;
        const int segs = (H + rows - 1) / rows;
        const long long items = base_items * segs;
        for (int w = wmax; w >= wmin; w -= 8) {
            const long long per = (items + w - 1) / w;
            const double balance = (double)items / (double)(per * w);
            const double occ = (double)w / (double)wmax;
            const double amort = (double)rows / (double)(rows + ring_rows - 1 + 2);  // ring prologue per item
            const double score = balance * (0.5 + 0.5 * occ) * amort;
            if (score > best) { best = score; best_w = w; best_rows = rows; }
        }
    }
    AzC2wPlan p{};
    p.blocks_per_combo = best_w;
    p.hseg_rows = best_rows;
    p.nhseg = (H + best_rows - 1) / best_rows;
    p.nitems = base_items * p.nhseg;
    if (p.nitems < p.blocks_per_combo) p.blocks_per_combo = (int)((p.nitems + 7) & ~7LL);
    return p;
}

// az_conv3d_wgrad16s2.hip (stride-2 weight gradient): a step stages 3 planes x 8 new fine rows x 17 positions x 8 float4
// pieces.  Piece f -> plane pk, row j, position pp (fine x = 2 cw0 - 1 + pp) and the LDS row of the position inside a
// staged row: the ODD fine positions (pp even) are rows 0..8, the EVEN ones rows 9..16, so that tap kw of coarse position x
// reads row x (kw = 0), 9 + x (kw = 1), 1 + x (kw = 2).
#define AZ_S2W_FPOS 17
#define AZ_S2W_FROWQ (AZ_S2W_FPOS * 8)
#define AZ_S2W_NFQ (3 * 8 * AZ_S2W_FROWQ)
#define AZ_S2W_RING 17
AZ_HD bool az_s2w_fine_piece(int f, int &pk, int &j, int &pp, int &lrow) {
    pk = f / (8 * AZ_S2W_FROWQ);
    const int g = f - pk * (8 * AZ_S2W_FROWQ);
    j = g / AZ_S2W_FROWQ;
    pp = (g - j * AZ_S2W_FROWQ) >> 3;
    lrow = (pp & 1) ? 9 + (pp >> 1) : (pp >> 1);
    return f < AZ_S2W_NFQ;
}
AZ_HD int az_s2w_tap_row(int kw) { return kw == 0 ? 0 : kw == 1 ? 9 : 1; }
// ring slot of fine row fr >= -1 (17 slots: the 9 rows a step reads + the 8 it writes for the next one)
AZ_HD int az_s2w_ring_slot(int fr) { return (fr + 1) % AZ_S2W_RING; }
// column -> (coarse depth, 8-position chunk, batch); consecutive columns = consecutive depths of one chunk
AZ_HD void az_s2w_col_decode(long long col, int Dc, int nwchunk, int &cd, int &wc, int &b) {
    cd = (int)(col % Dc); col /= Dc;
    wc = (int)(col % nwchunk);
    b = (int)(col / nwchunk);
}

// a tensor slice addressed through one 32-bit buffer offset must stay below the out-of-range marker the kernels use
inline bool az_fits_buffer_offset(long long bytes) { return bytes > 0 && bytes < 0xffffff00LL; }
