// CPU sweep of the launch arithmetic the HIP launches use (activezero_amd/csrc/az_launch_math.h), built with
// g++ -fsanitize=address,undefined by tests/test_launch_math_cpu.py.  Exit code 0 = every property held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../activezero_amd/csrc/az_launch_math.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { std::printf("FAIL %s:%d: %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

int main() {
    // 1. the XCD map is a bijection of [0, nblk)
    for (int nblk = 1; nblk <= 5000; nblk += (nblk < 600 ? 1 : 37)) {
        std::vector<char> seen(nblk, 0);
        for (int b = 0; b < nblk; ++b) {
            const int l = az_xcd_map(b, nblk);
            CHECK(l >= 0 && l < nblk, "nblk %d bid %d -> %d", nblk, b, l);
            if (l >= 0 && l < nblk) { CHECK(!seen[l], "nblk %d: %d hit twice", nblk, l); seen[l] = 1; }
        }
    }
    // 2. depth segments cover [0, Do) exactly; every workgroup decodes to a valid (patch, segment, batch), all distinct
    const int dims[][4] = {{1, 1, 1, 1}, {4, 48, 136, 240}, {4, 24, 68, 120}, {1, 3, 9, 33}, {2, 5, 7, 19}, {8, 1, 272, 480},
                           {1, 48, 136, 240}, {3, 47, 131, 239}, {6, 12, 34, 60}, {1, 192, 8, 16}, {16, 2, 300, 17}};
    for (const auto &d : dims)
        for (int forced = 0; forced <= 7; forced += (forced ? 3 : 1)) {
            const int B = d[0], Do = d[1], H = d[2], W = d[3];
            const int tiles_y = (H + 3) / 4, tiles_x = (W + 15) / 16, tyb = (tiles_y + 1) / 2;
            int nseg = -1, seg_len = -1;
            az_roll_segments((long long)B * tyb * tiles_x, Do, forced, nseg, seg_len);
            CHECK(nseg >= 1 && seg_len >= 1 && seg_len <= Do, "B%d Do%d: nseg %d len %d", B, Do, nseg, seg_len);
            CHECK((long long)nseg * seg_len >= Do && (long long)(nseg - 1) * seg_len < Do, "Do %d nseg %d len %d", Do, nseg, seg_len);
            const long long blocks = (long long)B * nseg * tyb * tiles_x;
            if (blocks > 200000) continue;
            std::vector<char> seen((size_t)blocks, 0);
            for (int bid = 0; bid < (int)blocks; ++bid) {
                int tix, tiy, seg, b;
                az_roll_decode(az_xcd_map(bid, (int)blocks), tiles_x, tyb, nseg, tix, tiy, seg, b);
                CHECK(tix >= 0 && tix < tiles_x && tiy >= 0 && tiy < tyb && seg >= 0 && seg < nseg && b >= 0 && b < B,
                      "decode (%d,%d,%d,%d) of (%d,%d,%d,%d)", tix, tiy, seg, b, tiles_x, tyb, nseg, B);
                const long long id = (((long long)b * nseg + seg) * tyb + tiy) * tiles_x + tix;
                if (id >= 0 && id < blocks) { CHECK(!seen[(size_t)id], "work item %lld twice", id); seen[(size_t)id] = 1; }
                const int d0 = seg * seg_len, d1 = d0 + seg_len < Do ? d0 + seg_len : Do;
                CHECK(d0 < d1 && d1 <= Do, "segment [%d, %d) of %d", d0, d1, Do);
            }
        }
    // 2b. coarse-depth segments of the transposed depth-rolling kernel; its workgroups decode like the stride-1 kernel's
    for (const auto &d : dims) {
        const int B = d[0], Di = d[1], H = d[2], W = d[3];
        const int tiles_y = (H + 3) / 4, tiles_x = (W + 15) / 16, tyb = (tiles_y + 1) / 2;
        int nseg = -1, seg_len = -1;
        az_t2roll_segments((long long)B * tyb * tiles_x, Di, nseg, seg_len);
        CHECK(nseg >= 1 && seg_len >= 1 && seg_len <= Di && (long long)nseg * seg_len >= Di && (long long)(nseg - 1) * seg_len < Di,
              "t2roll B%d Di%d: nseg %d len %d", B, Di, nseg, seg_len);
        for (int seg = 0; seg < nseg; ++seg) {  // every segment owns at least one coarse plane (the kernel's c0 < c1)
            const int c0 = seg * seg_len, c1 = c0 + seg_len < Di ? c0 + seg_len : Di;
            CHECK(c0 < c1, "t2roll empty segment %d of %d (len %d, Di %d)", seg, nseg, seg_len, Di);
        }
    }
    // 2c. output-depth segments of the stride-2 depth-rolling kernel (8 x 16 coarse patches); its workgroups decode with the
    //     same function, every (patch, segment, batch) once
    for (const auto &d : dims)
        for (int forced = 0; forced <= 7; forced += (forced ? 3 : 1)) {
            const int B = d[0], Do = (d[1] - 1) / 2 + 1, Ho = (d[2] - 1) / 2 + 1, Wo = (d[3] - 1) / 2 + 1;
            const int ty = (Ho + 7) / 8, tx = (Wo + 15) / 16;
            int nseg = -1, seg_len = -1;
            az_s2roll_segments((long long)B * ty * tx, Do, forced, nseg, seg_len);
            CHECK(nseg >= 1 && seg_len >= 1 && seg_len <= Do && (long long)nseg * seg_len >= Do && (long long)(nseg - 1) * seg_len < Do,
                  "s2roll B%d Do%d: nseg %d len %d", B, Do, nseg, seg_len);
            const long long blocks = (long long)B * nseg * ty * tx;
            std::vector<char> seen((size_t)blocks, 0);
            for (int bid = 0; bid < (int)blocks; ++bid) {
                int tix, tiy, seg, b;
                az_roll_decode(az_xcd_map(bid, (int)blocks), tx, ty, nseg, tix, tiy, seg, b);
                CHECK(tix >= 0 && tix < tx && tiy >= 0 && tiy < ty && seg >= 0 && seg < nseg && b >= 0 && b < B, "s2roll decode");
                const long long id = (((long long)b * nseg + seg) * ty + tiy) * tx + tix;
                if (id >= 0 && id < blocks) { CHECK(!seen[(size_t)id], "s2roll work item %lld twice", id); seen[(size_t)id] = 1; }
                CHECK(seg * seg_len < Do, "s2roll empty segment %d", seg);
            }
        }
    // 3. image segments of the 2-D batch-walking kernel
    for (int N = 1; N <= 64; ++N)
        for (long long patches = 1; patches <= 4096; patches *= 3) {
            int nseg = -1, len = -1;
            az_c2r_segments(patches, N, nseg, len);
            CHECK(nseg >= 1 && len >= 1 && (long long)nseg * len >= N && (long long)(nseg - 1) * len < N, "N %d: %d x %d", N, nseg, len);
        }
    // 4. slab staging: the kernels' incremental (sy, sx) stepping equals the closed form and stays inside the slab
    for (int tid = 0; tid < 256; ++tid) {
        int sy = 0, sx = tid >> 3;
        if (sx >= AZ_R_SX) { sx -= AZ_R_SX; ++sy; }
        for (int it = 0; it < (AZ_R_NQ + 255) / 256; ++it) {
            int cy, cx;
            const bool live = az_roll_piece(tid, it, cy, cx);
            if (live) {
                CHECK(cy == sy && cx == sx, "tid %d it %d: stepped (%d,%d) closed form (%d,%d)", tid, it, sy, sx, cy, cx);
                CHECK(cy >= 0 && cy < AZ_R_SY && cx >= 0 && cx < AZ_R_SX, "tid %d it %d outside the slab", tid, it);
            }
            sx += 14; ++sy;
            if (sx >= AZ_R_SX) { sx -= AZ_R_SX; ++sy; }
        }
    }
    // every live piece index is hit exactly once
    {
        std::vector<char> seen(AZ_R_NQ, 0);
        for (int tid = 0; tid < 256; ++tid)
            for (int it = 0; it < (AZ_R_NQ + 255) / 256; ++it) {
                int cy, cx;
                if (!az_roll_piece(tid, it, cy, cx)) continue;
                const int q = (cy * AZ_R_SX + cx) * 8 + (tid & 7);
                CHECK(q >= 0 && q < AZ_R_NQ && !seen[q], "piece %d twice or outside", q);
                if (q >= 0 && q < AZ_R_NQ) seen[q] = 1;
            }
        for (int q = 0; q < AZ_R_NQ; ++q) CHECK(seen[q], "piece %d never staged", q);
    }
    // 5. persistent workgroups of the weight-gradient kernel
    for (long long ncols = 1; ncols <= 100000; ncols = ncols * 5 / 3 + 1)
        for (int ntiles = 1; ntiles <= 4; ntiles *= 2)
            for (int cap = 0; cap <= 300; cap += 150) {
                const int slots = 512 / ntiles;
                const int w = az_wgrad16_workgroups(ncols, slots, ntiles, cap);
                CHECK(w >= 1 && w <= slots && (w <= ncols || ncols < 1), "ncols %lld slots %d -> %d", ncols, slots, w);
                if (cap > 0) CHECK(w <= cap, "cap %d -> %d", cap, w);
            }
    // 6. the 32-bit buffer-offset guard
    CHECK(az_fits_buffer_offset(1) && az_fits_buffer_offset(0xfffffeffLL) && !az_fits_buffer_offset(0xffffff00LL) &&
          !az_fits_buffer_offset(1LL << 33) && !az_fits_buffer_offset(0), "buffer offset guard");
    // 7. stride-2 weight gradient (az_conv3d_wgrad16s2.hip): staging pieces, tap rows, ring slots, column walk, offsets
    {
        // every (plane, row, position, float4) of a step's fine set is one piece; the LDS rows of a staged row are a permutation
        std::vector<char> seen(AZ_S2W_NFQ, 0);
        for (int f = 0; f < AZ_S2W_NFQ + 600; ++f) {
            int pk, j, pp, lrow;
            const bool live = az_s2w_fine_piece(f, pk, j, pp, lrow);
            CHECK(live == (f < AZ_S2W_NFQ), "piece %d liveness", f);
            if (!live) continue;
            CHECK(pk >= 0 && pk < 3 && j >= 0 && j < 8 && pp >= 0 && pp < AZ_S2W_FPOS && lrow >= 0 && lrow < AZ_S2W_FPOS, "piece %d -> %d %d %d %d", f, pk, j, pp, lrow);
            const int id = ((pk * 8 + j) * AZ_S2W_FPOS + pp) * 8 + (f & 7);
            CHECK(id == f && !seen[f], "piece %d is not its own index (%d)", f, id);
            seen[f] = 1;
        }
        char rows[AZ_S2W_FPOS] = {0};
        for (int pp = 0; pp < AZ_S2W_FPOS; ++pp) {
            int pk, j, p2, lrow;
            az_s2w_fine_piece(pp * 8, pk, j, p2, lrow);
            CHECK(p2 == pp && !rows[lrow], "LDS row %d of position %d taken", lrow, pp);
            rows[lrow] = 1;
            // tap kw of coarse position x reads fine position offset pp = 2x + kw: its row must be tap_row(kw) + x
            for (int kw = 0; kw < 3; ++kw)
                if ((pp - kw) >= 0 && (pp - kw) % 2 == 0 && (pp - kw) / 2 < 8)
                    CHECK(lrow == az_s2w_tap_row(kw) + (pp - kw) / 2, "pp %d kw %d: row %d", pp, kw, lrow);
        }
        // ring: the 9 rows step s reads and the 8 rows it writes for step s+1 sit in 17 distinct slots
        for (int s2 = 0; s2 < 200; ++s2) {
            char slot[AZ_S2W_RING] = {0};
            for (int fr = 8 * s2 - 1; fr <= 8 * s2 + 15; ++fr) {
                const int sl = az_s2w_ring_slot(fr);
                CHECK(sl >= 0 && sl < AZ_S2W_RING && !slot[sl], "step %d row %d: slot %d", s2, fr, sl);
                if (sl >= 0 && sl < AZ_S2W_RING) slot[sl] = 1;
            }
            // the kernel's per-lane form: (8s mod 17 + 2 oct + kh), minus 17 once
            for (int oct = 0; oct < 4; ++oct)
                for (int kh = 0; kh < 3; ++kh) {
                    int v = (8 * s2) % AZ_S2W_RING + 2 * oct + kh;
                    v = v >= AZ_S2W_RING ? v - AZ_S2W_RING : v;
                    CHECK(v == az_s2w_ring_slot(8 * s2 + 2 * oct - 1 + kh), "lane slot s %d oct %d kh %d", s2, oct, kh);
                }
        }
        // columns: the persistent workgroups (with the XCD map) visit every column once; global offsets of valid pieces,
        // formed the way the kernel forms them (32-bit wrap-around base + per-piece relative part), stay inside the tensor
        const int shapes[][7] = {{4, 24, 68, 120, 48, 136, 240}, {4, 12, 34, 60, 24, 68, 120}, {1, 2, 4, 7, 3, 7, 13}, {2, 3, 5, 18, 6, 10, 36},
                                 {8, 1, 136, 240, 1, 272, 480}, {1, 1, 1, 25, 2, 2, 50}};
        for (const auto &sh : shapes) {
            const int B = sh[0], Dc = sh[1], Wc = sh[3], Df = sh[4], Hf = sh[5], Wf = sh[6], CN = 32;
            const int nwchunk = (Wc + 7) / 8;
            const long long ncols = (long long)B * Dc * nwchunk;
            const int wgs = az_wgrad16_workgroups(ncols, 256, 1, 0);
            std::vector<char> seen_col((size_t)ncols, 0);
            for (int wgl = 0; wgl < wgs; ++wgl) {
                const int wg0 = (wgs & 7) ? wgl : az_xcd_map(wgl, wgs);
                for (long long col = wg0; col < ncols; col += wgs) {
                    CHECK(!seen_col[(size_t)col], "column %lld twice", col);
                    seen_col[(size_t)col] = 1;
                    int cd, wc, b;
                    az_s2w_col_decode(col, Dc, nwchunk, cd, wc, b);
                    CHECK(cd >= 0 && cd < Dc && wc >= 0 && wc < nwchunk && b >= 0 && b < B, "column %lld -> %d %d %d", col, cd, wc, b);
                    if (col % 7) continue;  // (offsets: a sample of the columns)
                    const unsigned vb_f = CN * 4u, plane_f = (unsigned)Hf * Wf * vb_f;
                    const long long vol_f = (long long)Df * plane_f;
                    const int cw0 = wc * 8;
                    const unsigned gbase = (unsigned)(2 * cd - 1) * plane_f + (unsigned)(2 * cw0 - 1) * vb_f;
                    for (int frow0 = 0; frow0 < Hf + 8; frow0 += 8)
                        for (int f = 0; f < AZ_S2W_NFQ; f += 5) {
                            int pk, j, pp, lrow;
                            az_s2w_fine_piece(f, pk, j, pp, lrow);
                            const int fd = 2 * cd - 1 + pk, fr = frow0 + j, fw = 2 * cw0 - 1 + pp;
                            if (fd < 0 || fd >= Df || fr >= Hf || fw < 0 || fw >= Wf) continue;
                            const unsigned rel = (unsigned)pk * plane_f + (unsigned)(j * Wf + pp) * vb_f + (unsigned)(f & 7) * 16u;
                            const unsigned off = gbase + (unsigned)frow0 * (unsigned)Wf * vb_f + rel;
                            const long long want = (long long)fd * plane_f + ((long long)fr * Wf + fw) * vb_f + (f & 7) * 16;
                            CHECK((long long)off == want && want + 16 <= vol_f, "offset %u vs %lld (volume %lld)", off, want, vol_f);
                        }
                }
            }
            for (long long c = 0; c < ncols; ++c) CHECK(seen_col[(size_t)c], "column %lld never walked", c);
        }
    }
    // 8. plans of the 2-D weight gradients (az_conv2d_wgrad16.hip, az_conv2d_wgrad.hip): row segments tile [0, H), the
    //    persistent workgroups / static work lists visit every column / item exactly once
    {
        const int Bs[] = {1, 2, 3, 8, 13, 131}, Hs[] = {1, 2, 3, 5, 9, 13, 24, 37, 47, 64, 136, 271},
                  Ws[] = {1, 15, 16, 17, 22, 47, 53, 150, 240, 400, 12320};
        const int slot_counts[] = {768, 384, 192, 256};
        for (int B : Bs) for (int H : Hs) for (int W : Ws) {
            const int nwchunk = (W + 15) / 16;
            for (int slots : slot_counts) {
                const AzC2w16Plan p = az_c2w16_plan(B, H, W, slots);
                CHECK(p.seg_rows >= 2 && p.seg_rows % 2 == 0, "r16 B%d H%d W%d slots %d: seg_rows %d", B, H, W, slots, p.seg_rows);
                CHECK(p.nrseg >= 1 && p.nrseg <= 16 && (long long)p.nrseg * p.seg_rows >= H && (long long)(p.nrseg - 1) * p.seg_rows < H,
                      "r16 B%d H%d W%d slots %d: %d segments of %d rows", B, H, W, slots, p.nrseg, p.seg_rows);
                CHECK(p.ncols == (long long)B * nwchunk * p.nrseg, "r16 ncols %lld", p.ncols);
                CHECK(p.wgs >= 1 && p.wgs <= slots && p.wgs <= p.ncols, "r16 B%d H%d W%d slots %d: wgs %d of %lld columns", B, H, W, slots, p.wgs, p.ncols);
                if (p.ncols > 20000) continue;
                // the kernels' walk: workgroup wg takes columns wg, wg + wgs, ...; a column decodes to a non-empty row range
                std::vector<char> seen((size_t)p.ncols, 0);
                for (int wg = 0; wg < p.wgs; ++wg)
                    for (long long col = wg; col < p.ncols; col += p.wgs) {
                        CHECK(!seen[(size_t)col], "r16 column %lld twice", col);
                        seen[(size_t)col] = 1;
                        long long r = col;
                        const int rs = (int)(r % p.nrseg); r /= p.nrseg;
                        const int wc = (int)(r % nwchunk), b = (int)(r / nwchunk);
                        const int h0 = rs * p.seg_rows, h1 = h0 + p.seg_rows < H ? h0 + p.seg_rows : H;
                        CHECK(b >= 0 && b < B && wc < nwchunk && h0 % 2 == 0 && h0 < h1, "r16 column %lld -> b %d chunk %d rows [%d, %d)", col, b, wc, h0, h1);
                    }
                for (long long c = 0; c < p.ncols; ++c) CHECK(seen[(size_t)c], "r16 column %lld never walked", c);
            }
            for (int mt = 1; mt <= 2; ++mt) for (int nt = 1; nt <= 2; ++nt)
                for (int cm = 32 * mt; cm <= 192; cm += 64 * mt) for (int cn = 32 * nt; cn <= 192; cn += 64 * nt)
                    for (int ring = 1; ring <= 5; ring += 2) {
                        const int ncombo = (cm / (32 * mt)) * (cn / (32 * nt));
                        const AzC2wPlan p = az_c2w_plan(B, H, W, mt, nt, ncombo, ring);
                        CHECK(p.hseg_rows >= 1 && p.nhseg >= 1 && (long long)p.nhseg * p.hseg_rows >= H && (long long)(p.nhseg - 1) * p.hseg_rows < H,
                              "w2 B%d H%d W%d %dx%d: %d segments of %d rows", B, H, W, mt, nt, p.nhseg, p.hseg_rows);
                        CHECK(p.nitems == (long long)B * nwchunk * p.nhseg, "w2 nitems %lld", p.nitems);
                        CHECK(p.blocks_per_combo >= 8 && p.blocks_per_combo % 8 == 0, "w2 blocks per combo %d", p.blocks_per_combo);
                        CHECK((long long)p.blocks_per_combo * ncombo <= 2048 / (mt * nt) + 8LL * ncombo, "w2 grid %d x %d", p.blocks_per_combo, ncombo);
                        // the kernel's block -> (combo, list index) map: every (combo, index) once, the lists cover the items
                        const int nblk = p.blocks_per_combo * ncombo;
                        std::vector<char> taken((size_t)nblk, 0);
                        for (int bid = 0; bid < nblk; ++bid) {
                            const int grp = bid / (8 * ncombo), rem = bid % (8 * ncombo);
                            const int combo = rem >> 3, widx = grp * 8 + (rem & 7);
                            CHECK(combo < ncombo && widx < p.blocks_per_combo, "w2 block %d -> combo %d list %d", bid, combo, widx);
                            const int id = combo * p.blocks_per_combo + widx;
                            if (id >= 0 && id < nblk) { CHECK(!taken[(size_t)id], "w2 list %d twice", id); taken[(size_t)id] = 1; }
                        }
                    }
        }
    }
    // 9. the 32 -> 1 classifier convolutions (az_conv3d_c1.hip).  Forward: the depth segments tile [0, D) -- every plane is
    //    written by exactly one workgroup of a patch -- and no segment length has a lower cost.  Weight gradient: the strided
    //    walk of at most 2048 workgroups visits every (batch, plane, tile) item exactly once and decodes it inside the volume
    {
        const long long patch_counts[] = {1, 2, 3, 7, 30, 48, 100, 255, 256, 257, 383, 384, 385, 767, 768, 769, 1000, 1536, 2040, 3000, 4080, 6528};
        for (int D = 1; D <= 2100; ++D)
            for (long long patches : patch_counts) {
                const int dseg = az_c1_fwd_dseg(patches, D);
                CHECK(dseg >= 1 && dseg <= D, "c1 patches %lld D %d: dseg %d", patches, D, dseg);
                if (dseg < 1) continue;
                const int nseg = (D + dseg - 1) / dseg;
                CHECK((long long)nseg * dseg >= D && (long long)(nseg - 1) * dseg < D, "c1 D %d: %d segments of %d", D, nseg, dseg);
                std::vector<char> written((size_t)D, 0);
                for (int seg = 0; seg < nseg; ++seg) {  // the kernel's d0, d1 of blockIdx.y = seg
                    const int d0 = seg * dseg, d1 = d0 + dseg < D ? d0 + dseg : D;
                    CHECK(d0 < d1, "c1 D %d dseg %d: empty segment %d", D, dseg, seg);
                    for (int od = d0; od < d1; ++od) { CHECK(!written[(size_t)od], "c1 plane %d twice", od); written[(size_t)od] = 1; }
                }
                for (int od = 0; od < D; ++od) CHECK(written[(size_t)od], "c1 D %d dseg %d: plane %d never written", D, dseg, od);
                const long long cost = az_c1_fwd_cost(patches, D, dseg);
                for (int other = 1; other <= D; ++other) {
                    const long long c = az_c1_fwd_cost(patches, D, other);
                    CHECK(c >= cost, "c1 patches %lld D %d: dseg %d costs %lld, %d costs %lld", patches, D, dseg, cost, other, c);
                    if (c == cost && (D + other - 1) / other != nseg) CHECK(other < dseg, "c1 D %d: the longer equal %d not taken", D, other);
                }
            }
        // (values the launches had before the selection moved here)
        CHECK(az_c1_fwd_dseg(17LL * 15, 48) == 16 && az_c1_fwd_dseg(3LL * 5 * 9, 7) == 2 && az_c1_fwd_dseg(8LL * 10, 20) == 3 &&
              az_c1_fwd_dseg(1, 2050) == 3 && az_c1_fwd_dseg(768, 3) == 3 && az_c1_fwd_dseg(2LL * 15, 48) == 2 &&
              az_c1_fwd_dseg(3LL * 2 * 5, 5) == 1, "c1 forward segment lengths changed");
        const int shapes[][4] = {{1, 1, 1, 1}, {1, 2050, 3, 5}, {768, 3, 8, 16}, {1, 48, 16, 240}, {3, 7, 40, 130}, {2, 5, 7, 13}, {1, 48, 136, 240},
                                 {5, 9, 17, 65}, {1, 2047, 8, 32}, {1, 2048, 8, 32}, {1, 2049, 9, 33}, {3, 1367, 1, 1}, {65535, 1, 1, 1}};
        for (const auto &sh : shapes) {
            const int B = sh[0], D = sh[1], H = sh[2], W = sh[3];
            const int tiles_x = (W + 31) / 32, tiles_y = (H + 7) / 8;
            const long long ntiles = az_c1_wgrad_tiles(B, D, H, W);
            const int grid = az_c1_wgrad_grid(ntiles);
            CHECK(ntiles == (long long)B * D * tiles_y * tiles_x, "c1 wgrad tiles %lld", ntiles);
            CHECK(grid >= 1 && grid <= AZ_C1_WGRAD_MAX_GRID && grid <= ntiles && (grid == ntiles || grid == AZ_C1_WGRAD_MAX_GRID),
                  "c1 wgrad grid %d of %lld tiles", grid, ntiles);
            std::vector<char> seen((size_t)ntiles, 0);
            for (int blk = 0; blk < grid; ++blk)
                for (long long item = blk; item < ntiles; item += grid) {
                    CHECK(!seen[(size_t)item], "c1 wgrad item %lld twice", item);
                    seen[(size_t)item] = 1;
                    long long r = item;  // the kernel's decode
                    const int tx0 = (int)(r % tiles_x) * 32; r /= tiles_x;
                    const int ty0 = (int)(r % tiles_y) * 8; r /= tiles_y;
                    const int od = (int)(r % D), b = (int)(r / D);
                    CHECK(tx0 < W && ty0 < H && od >= 0 && od < D && b >= 0 && b < B, "c1 wgrad item %lld -> (%d, %d, %d, %d)", item, b, od, ty0, tx0);
                }
            for (long long i = 0; i < ntiles; ++i) CHECK(seen[(size_t)i], "c1 wgrad item %lld never visited", i);
        }
        for (long long nt = 1; nt <= 5000; ++nt) {
            const int grid = az_c1_wgrad_grid(nt);
            CHECK(grid == (nt < 2048 ? nt : 2048), "c1 wgrad grid %d of %lld", grid, nt);
            long long visited = 0;
            for (int blk = 0; blk < grid; ++blk) visited += (nt - blk + grid - 1) / grid;
            CHECK(visited == nt, "c1 wgrad: %lld of %lld items visited", visited, nt);
        }
    }
    // C layout of the two MFMA shapes the weight-gradient kernels flush: every (lane, register) is a distinct (m, n), all of the tile
    {
        std::vector<char> seen32(32 * 32, 0), seen16(16 * 16, 0);
        for (int lane = 0; lane < 64; ++lane) {
            for (int rg = 0; rg < 16; ++rg) {
                const int m = az_mfma32_c_row(lane, rg), n = az_mfma32_c_col(lane);
                CHECK(m >= 0 && m < 32 && n >= 0 && n < 32, "32x32 C: lane %d reg %d -> (%d, %d)", lane, rg, m, n);
                if (m >= 0 && m < 32 && n >= 0 && n < 32) { CHECK(!seen32[m * 32 + n], "32x32 C: (%d, %d) twice", m, n); seen32[m * 32 + n] = 1; }
            }
            for (int r = 0; r < 4; ++r) {
                const int m = az_mfma16_c_row(lane, r), n = az_mfma16_c_col(lane);
                CHECK(m >= 0 && m < 16 && n >= 0 && n < 16, "16x16 C: lane %d reg %d -> (%d, %d)", lane, r, m, n);
                if (m >= 0 && m < 16 && n >= 0 && n < 16) { CHECK(!seen16[m * 16 + n], "16x16 C: (%d, %d) twice", m, n); seen16[m * 16 + n] = 1; }
            }
        }
        for (int i = 0; i < 32 * 32; ++i) CHECK(seen32[i], "32x32 C: element %d never held", i);
        for (int i = 0; i < 16 * 16; ++i) CHECK(seen16[i], "16x16 C: element %d never held", i);
    }
    // The row-half swap of the r16 weight-gradient images: what staging writes for (k row, channel) is what the transposing read
    // of that (k row, channel) addresses, and the two octets of a 32-lane half read different 32-byte halves of the bank period.
    {
        for (int ch0 = 0; ch0 <= 16; ch0 += 16)
            for (int lane = 0; lane < 64; ++lane) {
                const int oct = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
                const AzW16Lanes g = az_w16_lanes(lane, ch0, ch0);
                // coarse: k row 8 oct + tq (+ 4 for the second half of a fragment); the piece of channels ch0 + 4 tp ..
                CHECK((int)g.a_lane == az_w16_piece_off(8 * oct + tq, (ch0 + 4 * tp) / 4), "a_lane of lane %d", lane);
                CHECK(az_w16_piece_off(8 * oct + tq + 4, (ch0 + 4 * tp) / 4) == (int)g.a_lane + 4 * AZ_W16_ROWB, "a_lane + 4 rows, lane %d", lane);
                CHECK(g.rp == (oct >> 1), "rp of lane %d", lane);
                for (int kw = 0; kw < 3; ++kw)
                    for (int h2 = 0; h2 < 2; ++h2) {
                        const int row = 8 * (oct & 1) + tq + kw + 4 * h2;  // position + tap shift inside the 18-position row
                        CHECK(row < 18, "fine row %d of lane %d", row, lane);
                        CHECK((int)g.b_off[kw][h2] == az_w16_piece_off(row, (ch0 + 4 * tp) / 4), "b_off[%d][%d] of lane %d", kw, h2, lane);
                    }
                if (!(oct & 1)) {  // the other octet of this 32-lane half: same tq, tp
                    const AzW16Lanes o = az_w16_lanes(lane + 16, ch0, ch0);
                    CHECK(((g.a_lane ^ o.a_lane) & 32u) != 0, "a: octets of lane %d share a half", lane);
                    for (int kw = 0; kw < 3; ++kw)
                        for (int h2 = 0; h2 < 2; ++h2)
                            CHECK(((g.b_off[kw][h2] ^ o.b_off[kw][h2]) & 32u) != 0, "b[%d][%d]: octets of lane %d share a half", kw, h2, lane);
                }
            }
        // staging covers every 8-byte piece of a 32-row image exactly once
        std::vector<char> seen(32 * AZ_W16_ROWB / 8, 0);
        for (int row = 0; row < 32; ++row)
            for (int q = 0; q < 8; ++q) {
                const int off = az_w16_piece_off(row, q);
                CHECK(off >= 0 && off < 32 * AZ_W16_ROWB && off % 8 == 0 && off / AZ_W16_ROWB == row && !seen[off / 8], "piece (%d, %d) -> %d", row, q, off);
                if (off >= 0 && off < 32 * AZ_W16_ROWB) seen[off / 8] = 1;
            }
    }
    // The gather kernels' block -> tile map (az_conv3d.hip, az_conv3d_m128.hip, az_conv3d_t2.hip): with every map mode and
    // both band heights the blocks of a launch decode into range and hit every (tix, tiy, td, b) exactly once; map mode 0 is
    // the plain mixed radix of the block id.  Row counts: those of `dims` and every residue of rows_y % band, rows_y < band
    // and rows_y == 1 among them.
    {
        std::vector<std::vector<int>> cases;  // B, Dt, rows_y, tiles_x
        for (const auto &d : dims) {
            cases.push_back({d[0], d[1], (d[2] + 3) / 4, (d[3] + 15) / 16});               // 4-row tiles
            cases.push_back({d[0], d[1], ((d[2] + 3) / 4 + 1) / 2, (d[3] + 15) / 16});     // 8-row tile rows (m128)
        }
        for (int rows = 1; rows <= 13; ++rows)
            for (int Dt = 1; Dt <= 5; Dt += 2) { cases.push_back({1, Dt, rows, 3}); cases.push_back({3, Dt, rows, 1}); }
        for (const auto &c : cases)
            for (int map_mode = 0; map_mode <= 2; ++map_mode)
                for (int band = 2; band <= 4; band += 2) {
                    const int B = c[0], Dt = c[1], rows_y = c[2], tiles_x = c[3];
                    const long long nblk = (long long)B * Dt * rows_y * tiles_x;
                    if (nblk > 400000) continue;
                    std::vector<char> seen((size_t)nblk, 0);
                    for (int bid = 0; bid < (int)nblk; ++bid) {
                        int tix = -1, tiy = -1, td = -1, b = -1;
                        az_conv_tile_decode(map_mode >= 1 ? az_xcd_map(bid, (int)nblk) : bid, map_mode, band, tiles_x, rows_y, Dt, tix, tiy, td, b);
                        const bool in = tix >= 0 && tix < tiles_x && tiy >= 0 && tiy < rows_y && td >= 0 && td < Dt && b >= 0 && b < B;
                        CHECK(in, "tile map %d band %d: block %d of (%d,%d,%d,%d) -> (%d,%d,%d,%d)", map_mode, band, bid, B, Dt, rows_y, tiles_x, b, td, tiy, tix);
                        if (!in) continue;
                        const long long id = (((long long)b * Dt + td) * rows_y + tiy) * tiles_x + tix;
                        CHECK(!seen[(size_t)id], "tile map %d band %d: tile %lld of (%d,%d,%d,%d) twice", map_mode, band, id, B, Dt, rows_y, tiles_x);
                        seen[(size_t)id] = 1;
                        if (map_mode == 0) CHECK(id == bid, "tile map 0: block %d -> tile %lld", bid, id);
                    }
                }
    }
    // The 24-dword slab image (az_conv3d_m128.hip, az_conv3d_t2.hip, az_conv2d.hip): the dword the commit writes for (voxel,
    // chunk channel, part) is the dword the fragment element that must hold that channel reads -- lane: row = lane & 31 =
    // voxel (row >> 3, row & 7) of its 4x8 tile, half = lane >> 5; element e of the 16-byte read <-> channel 8 half + e, two
    // per dword -- and the offsets are distinct and inside the slab.  Slabs: 10 x 18 (m128, conv2d 3x3), 5 x 17 (t2), 12 x 20.
    {
        const int slabs[][2] = {{10, 18}, {5, 17}, {12, 20}, {8, 16}};
        const int pitch = 20;
        for (const auto &sl : slabs) {
            const int SY = sl[0], SX = sl[1];
            std::vector<char> seen((size_t)SY * pitch * AZ_S24_VS, 0);
            for (int sy = 0; sy < SY; ++sy)
                for (int sx = 0; sx < SX; ++sx)
                    for (int part = 0; part < 3; ++part)
                        for (int j = 0; j < 4; ++j) {  // the 8-byte piece of channels 4j .. 4j + 3
                            const int off = az_s24_write_off(sy, sx, j, pitch) + 8 * part;
                            const bool in = off >= 0 && off + 1 < SY * pitch * AZ_S24_VS && off % 2 == 0;
                            CHECK(in, "slab %dx%d: piece (%d,%d,%d,%d) at %d", SY, SX, sy, sx, part, j, off);
                            if (!in) continue;
                            CHECK(!seen[(size_t)off] && !seen[(size_t)off + 1], "slab %dx%d: dword %d written twice", SY, SX, off);
                            seen[(size_t)off] = seen[(size_t)off + 1] = 1;
                        }
            // every lane of a fragment whose tile sits at (dy, dx) inside the slab
            for (int dy = 0; dy + 4 <= SY; ++dy)
                for (int dx = 0; dx + 8 <= SX; ++dx)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int part = 0; part < 3; ++part)
                            for (int e = 0; e < 8; ++e) {
                                const int row = lane & 31, half = lane >> 5, rty = row >> 3, rtx = row & 7;
                                const int rd = az_s24_read_base(rty, rtx, half, dy & 1, pitch) + (dy * pitch + dx) * AZ_S24_VS + 8 * part + e / 2;
                                const int ch = 8 * half + e;
                                const int wr = az_s24_write_off(rty + dy, rtx + dx, ch >> 2, pitch) + 8 * part + (ch & 3) / 2;
                                CHECK(rd == wr, "slab %dx%d: lane %d at (%d,%d) part %d element %d reads %d, channel %d is at %d", SY, SX, lane, dy, dx,
                                      part, e, rd, ch, wr);
                            }
        }
    }
    std::printf("launch math: %d failures\n", fails);
    return fails ? 1 : 0;
}
