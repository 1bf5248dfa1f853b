// sp_jpeg_prog.h - the entropy core of the progressive JPEG decoder: the four block procedures of T.81 G.1.2 / G.2 with libjpeg's
// (jdphuff) arithmetic, and the walk over one restart segment of one scan, as inline functions shared by jpeg_prog_entropy_kernel
// (device) and a stand-alone CPU program that runs them under the sanitizers (tests/jpeg_prog_core_main.cpp).  Plain C++ on top of the
// bit reader and the Huffman tables of sp_jpeg.h, whose rules hold here too: no byte at or past `end` is read, missing bits read as zeros
// and set a status bit, the first error ends the segment.
//
// Block geometry - the part that is easy to get wrong:
//   - a scan of two or three components is INTERLEAVED over the frame's MCU grid (mcus_x x mcus_y, h x v blocks per component per MCU),
//     like the baseline scan; that includes a two-component scan of a three-component file;
//   - a scan of ONE component is NOT interleaved: its "MCU" is one block, and it covers ceil(comp_width / 8) x ceil(comp_height / 8)
//     blocks with comp_width = ceil(width * h / hmax) - not the MCU-padded grid; its restart interval counts blocks, and the padding
//     blocks keep whatever the interleaved scans gave them;
//   - the arena layout is the baseline one: component after component, each a row-major grid of (mcus_x h) x (mcus_y v) blocks.
// Every block index is formed from the host-checked descriptor alone (MCU < the scan's MCU count, which the grid bounds), every
// coefficient index is a zigzag position k <= Se <= 63: whatever the bytes say, nothing leaves the image's own coefficient region.
#pragma once
#include "simple_pose_hip.h"
#include "sp_jpeg.h"

// One scan over one image.  Per-slot values as named scalars (slot j = the scan's j-th component), not arrays: in the kernel they stay in
// registers.
struct sp_jpeg_prog_geom {
    int32_t ncomp;                       // components in the scan, 1..3
    int32_t grid_w, mcus;                // MCUs per row and in all, of THIS scan (blocks for a one-component scan)
    int32_t first0, bw0, h0, v0;         // slot j: first block of its component in the image's region, blocks per arena row, blocks per MCU
    int32_t first1, bw1, h1, v1;
    int32_t first2, bw2, h2, v2;
    int32_t ss, se, ah, al;
};

// `d` has passed sp_jpeg_geometry (host check).  The scan's own fields are clamped into their ranges, so a record that differs from the
// host-checked one still addresses the image's own blocks only.
SP_JPEG_HD void sp_jpeg_prog_geometry(const sp_jpeg_desc& d, const sp_jpeg_scan& s, sp_jpeg_prog_geom& g) {
    const int nc = d.components == 3 ? 3 : 1;
    g.ncomp = sp_jpeg_clampi(s.components, 1, nc);
    g.se = sp_jpeg_clampi(s.se, 0, 63);
    g.ss = sp_jpeg_clampi(s.ss, 0, g.se);
    g.ah = sp_jpeg_clampi(s.ah, 0, 13);
    g.al = sp_jpeg_clampi(s.al, 0, 13);
    const int hmax = d.h_samp[0], vmax = d.v_samp[0];
    const int bw_0 = d.mcus_x * d.h_samp[0], bw_1 = nc == 3 ? d.mcus_x * d.h_samp[1] : 0, bw_2 = nc == 3 ? d.mcus_x * d.h_samp[2] : 0;
    const int fst_1 = bw_0 * d.mcus_y * d.v_samp[0], fst_2 = fst_1 + (nc == 3 ? bw_1 * d.mcus_y * d.v_samp[1] : 0);
    const int c0 = sp_jpeg_clampi(s.comp[0], 0, nc - 1), c1 = sp_jpeg_clampi(s.comp[1], 0, nc - 1), c2 = sp_jpeg_clampi(s.comp[2], 0, nc - 1);
    g.first0 = c0 == 0 ? 0 : (c0 == 1 ? fst_1 : fst_2); g.bw0 = c0 == 0 ? bw_0 : (c0 == 1 ? bw_1 : bw_2);
    g.first1 = c1 == 0 ? 0 : (c1 == 1 ? fst_1 : fst_2); g.bw1 = c1 == 0 ? bw_0 : (c1 == 1 ? bw_1 : bw_2);
    g.first2 = c2 == 0 ? 0 : (c2 == 1 ? fst_1 : fst_2); g.bw2 = c2 == 0 ? bw_0 : (c2 == 1 ? bw_1 : bw_2);
    if (g.ncomp == 1) {
        // not interleaved: one block per MCU over the component's own ceil(w / 8) x ceil(h / 8) blocks (<= its arena grid: the arena
        // row holds mcus_x * h blocks = a multiple of 8 samples that is >= comp_width)
        const int comp_w = (d.width * d.h_samp[c0] + hmax - 1) / hmax, comp_h = (d.height * d.v_samp[c0] + vmax - 1) / vmax;
        g.grid_w = (comp_w + 7) / 8;
        g.mcus = g.grid_w * ((comp_h + 7) / 8);
        g.h0 = g.v0 = 1;
        g.h1 = g.v1 = g.h2 = g.v2 = 0;
    } else {
        g.grid_w = d.mcus_x;
        g.mcus = d.mcus_x * d.mcus_y;
        g.h0 = d.h_samp[c0]; g.v0 = d.v_samp[c0];
        g.h1 = d.h_samp[c1]; g.v1 = d.v_samp[c1];
        g.h2 = g.ncomp == 3 ? d.h_samp[c2] : 0; g.v2 = g.ncomp == 3 ? d.v_samp[c2] : 0;
    }
}

// restart segments the scan has to have: ceil(MCUs / interval), 1 without restart markers
SP_JPEG_HD int sp_jpeg_prog_interval(const sp_jpeg_prog_geom& g, int restart_interval) { return restart_interval > 0 ? restart_interval : g.mcus; }

// Huffman tables the scan reads: a first DC scan one per component, an AC scan one, a DC refinement none
SP_JPEG_HD int sp_jpeg_prog_tables(const sp_jpeg_prog_geom& g) { return g.ss > 0 ? 1 : (g.ah ? 0 : g.ncomp); }

SP_JPEG_HD int16_t sp_jpeg_prog_i16(uint32_t v) { return (int16_t)(uint16_t)(v & 0xFFFFu); }

// ---- the four block procedures ------------------------------------------------------------------------------------------------------------
// DC, first pass: the difference is added to `pred` (per component, reset per restart segment); coef[0] = pred << Al, int16 wrap
SP_JPEG_HD void sp_jpeg_prog_dc_first(sp_jpeg_bits& b, const sp_jpeg_huff& dc, int al, int32_t& pred, int16_t* blk) {
    int s = sp_jpeg_huff_decode(dc, b);
    if (s > 15) { b.status |= SP_JPEG_ST_BAD_CODE; s = 0; }
    const int diff = sp_jpeg_extend(sp_jpeg_bits_get(b, s), s);
    pred = (int32_t)((uint32_t)pred + (uint32_t)diff);
    blk[0] = sp_jpeg_prog_i16((uint32_t)pred << al);
}

// DC, refinement: one raw bit
SP_JPEG_HD void sp_jpeg_prog_dc_refine(sp_jpeg_bits& b, int al, int16_t* blk) {
    if (sp_jpeg_bits_get(b, 1)) blk[0] = sp_jpeg_prog_i16((uint32_t)(uint16_t)blk[0] | (1u << al));
}

// AC, first pass.  `eobrun`: blocks of the segment still to end without a symbol (state of the segment, carried from block to block).
SP_JPEG_HD void sp_jpeg_prog_ac_first(sp_jpeg_bits& b, const sp_jpeg_huff& ac, int ss, int se, int al, int32_t& eobrun, int16_t* blk) {
    if (eobrun > 0) { eobrun -= 1; return; }
    for (int k = ss; k <= se && !b.status;) {
        const int rs = sp_jpeg_huff_decode(ac, b);
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            if (r == 15) { k += 16; continue; }                                   // ZRL
            eobrun = (1 << r) + sp_jpeg_bits_get(b, r) - 1;                       // this block and the next `eobrun` end here; <= 32767
            return;
        }
        k += r;
        if (k > se) { b.status |= SP_JPEG_ST_BAD_RUN; return; }
        const int v = sp_jpeg_extend(sp_jpeg_bits_get(b, sz), sz);
        blk[sp_jpeg_natural(k)] = sp_jpeg_prog_i16((uint32_t)v << al);
        k += 1;
    }
}

// one correction bit for an already non-zero coefficient
SP_JPEG_HD void sp_jpeg_prog_correct(sp_jpeg_bits& b, int p1, int16_t* c) {
    if (sp_jpeg_bits_get(b, 1) && ((int)*c & p1) == 0) *c = sp_jpeg_prog_i16((uint32_t)((int)*c + (*c >= 0 ? p1 : -p1)));
}

// AC, refinement.  A run counts only coefficients that are still zero; every non-zero coefficient that is passed - while a run is
// skipped, after the block's EOB, inside an EOB run - reads one correction bit.
SP_JPEG_HD void sp_jpeg_prog_ac_refine(sp_jpeg_bits& b, const sp_jpeg_huff& ac, int ss, int se, int al, int32_t& eobrun, int16_t* blk) {
    const int p1 = 1 << al;
    int k = ss;
    if (eobrun == 0) {
        for (; k <= se && !b.status; ++k) {
            const int rs = sp_jpeg_huff_decode(ac, b);
            int r = rs >> 4;
            const int sz = rs & 15;
            int value = 0;
            if (sz) {
                if (sz != 1) { b.status |= SP_JPEG_ST_BAD_CODE; return; }
                value = sp_jpeg_bits_get(b, 1) ? p1 : -p1;
            } else if (r != 15) {
                eobrun = (1 << r) + sp_jpeg_bits_get(b, r);                       // this block included: decremented below
                break;
            }
            for (; k <= se; ++k) {                                                // skip r zeros (ZRL: 15, then the 16th by the outer ++k)
                int16_t* c = blk + sp_jpeg_natural(k);
                if (*c != 0) sp_jpeg_prog_correct(b, p1, c);
                else if (--r < 0) break;
            }
            if (value) {
                if (k > se) { b.status |= SP_JPEG_ST_BAD_RUN; return; }
                blk[sp_jpeg_natural(k)] = (int16_t)value;
            }
        }
    }
    if (eobrun > 0) {
        for (; k <= se && !b.status; ++k) {
            int16_t* c = blk + sp_jpeg_natural(k);
            if (*c != 0) sp_jpeg_prog_correct(b, p1, c);
        }
        eobrun -= 1;
    }
}

// ---- one restart segment of one scan ----------------------------------------------------------------------------------------------------------
// MCUs [mcu_begin, mcu_end) of the scan (the caller clamps mcu_end to g.mcus) from the bytes [begin, end).  tabs: the scan's tables
// (sp_jpeg_prog_tables of them, luts filled).  coef: the image's coefficient region.  Returns the status bits.
SP_JPEG_HD int sp_jpeg_prog_segment(const uint8_t* begin, const uint8_t* end, const sp_jpeg_huff* tabs, const sp_jpeg_prog_geom& g, int mcu_begin, int mcu_end,
                                    int16_t* coef) {
    sp_jpeg_bits b;
    sp_jpeg_bits_init(b, begin, end);
    int32_t pred0 = 0, pred1 = 0, pred2 = 0, eobrun = 0;
    const int ss = g.ss, se = g.se, ah = g.ah, al = g.al, grid_w = g.grid_w;
    if (mcu_end > g.mcus) mcu_end = g.mcus;
    if (ss > 0) {
        // AC scan: one component, one block per MCU
        for (int mcu = mcu_begin; mcu < mcu_end && !b.status; ++mcu) {
            const int by = mcu / grid_w, bx = mcu - by * grid_w;
            int16_t* blk = coef + (size_t)(g.first0 + by * g.bw0 + bx) * 64;
            if (ah == 0) sp_jpeg_prog_ac_first(b, tabs[0], ss, se, al, eobrun, blk);
            else sp_jpeg_prog_ac_refine(b, tabs[0], ss, se, al, eobrun, blk);
        }
        return b.status;
    }
    // DC scan: the h x v blocks of each of the scan's components in MCU (mx, my); block < first + bw * (rows of the component)
    auto component = [&](int first, int bw, int h, int v, const sp_jpeg_huff& dc, int32_t& pred, int mx, int my) {
        for (int vy = 0; vy < v && !b.status; ++vy)
            for (int hx = 0; hx < h && !b.status; ++hx) {
                int16_t* blk = coef + (size_t)(first + (my * v + vy) * bw + mx * h + hx) * 64;
                if (ah == 0) sp_jpeg_prog_dc_first(b, dc, al, pred, blk);
                else sp_jpeg_prog_dc_refine(b, al, blk);
            }
    };
    for (int mcu = mcu_begin; mcu < mcu_end && !b.status; ++mcu) {
        const int my = mcu / grid_w, mx = mcu - my * grid_w;
        component(g.first0, g.bw0, g.h0, g.v0, tabs[0], pred0, mx, my);
        if (g.ncomp >= 2) component(g.first1, g.bw1, g.h1, g.v1, tabs[1], pred1, mx, my);
        if (g.ncomp == 3) component(g.first2, g.bw2, g.h2, g.v2, tabs[2], pred2, mx, my);
    }
    return b.status;
}
