// Tile plan of the fp32 GEMM (kernels.h GemmPlan): which kernel instantiation gemm() (gemm.hip) launches for a GemmArgs.  Host only,
// no launch and no HIP call, so that a selection rule can be changed and the shapes it moves seen at once (tests/golden/gemm_plans.txt).
#include "kernels.h"

namespace k2hip {

namespace {

GemmForce g_force;  // debug_force_gemm_cfg (tuning hook)

// the plan of table entry idx of a family; false when there is no such entry
bool entry(GemmFamily f, int idx, GemmPlan* p) {
    p->family = f;
    p->idx = idx;
    switch (f) {
#define X(i, bm, bn, wm, wn, bk_or_nst) case i: p->BM = bm; p->BN = bn; p->waves = (bm / wm) * (bn / wn); return true;
        case GemmFamily::REG: switch (idx) { K2_REG_TABLE(X) } return false;
        case GemmFamily::DMA: switch (idx) { K2_DMA_TABLE(X) } return false;
        case GemmFamily::PIPE: switch (idx) { K2_PIPE_TABLE(X) } return false;
        case GemmFamily::P16: switch (idx) { K2_P16_TABLE(X) } return false;
#undef X
        case GemmFamily::RING: {
            if (idx < 0 || idx >= (int)(sizeof(kRing) / sizeof(kRing[0]))) return false;
            const RingCfg& r = kRing[idx];
            p->BM = r.BM;
            p->BN = r.BN;
            p->waves = (r.BM / 32) * (r.BN / 32) * r.KS + r.LW + r.PF;
            return true;
        }
        case GemmFamily::SKINNY3: p->BM = 16; p->BN = 48; p->waves = 4; return idx == 0;
        case GemmFamily::SKINNY6: p->BM = 16; p->BN = 96; p->waves = 4; return idx == 0;
        case GemmFamily::SKINNY6_8: p->BM = 16; p->BN = 96; p->waves = 8; return idx == 0;
    }
    return false;
}

GemmPlan make(GemmFamily f, int idx, int ablate) {
    GemmPlan p;
    entry(f, idx, &p);
    p.ablate = ablate;
    return p;
}

// Small problems with more than a handful of columns (the streaming chunk step: 256 .. 2048 rows): small ring tiles with the
// K step split over four (two) wave groups of the workgroup put 4 - 8 waves on ~200 CUs and walk K in K / 128 (K / 64) steps
// through coalesced LDS-DMA tiles, where the 16-row skinny kernel re-reads the weight chunk M / 16 times straight into
// fragment layout (half-used cache lines; it is bound by the texture-address path, not by latency).  Choice by grid size,
// from tools/gemm_lab.py streaming: 17 % less GEMM time over the chunk step's shapes.  -1: none.
int small_ring_entry(int M, int N, int K) {
    const long long g32 = (long long)cdiv(M, 32) * cdiv(N, 32), g6432 = (long long)cdiv(M, 64) * cdiv(N, 32);
    if (K % 128 == 0 && g32 <= 256) return 16;     // 32x32 tiles, KS 4, 4 stages + L2 prefetch wave
    if (K % 128 == 0 && g6432 <= 256) return 17;   // 64x32 tiles, KS 4, 3 stages
    // K a multiple of 64 but not of 128 (the 256-wide stacks' feed-forward outputs: K = 576 / 960, and K = 192): 32x64 tiles, KS 2 --
    // round 4, tools/gemm_lab.py streaming-real: 1024 x 256 x 960 14.7 against 17.3 us (skinny),
    // x 576 10.4 against 12.2, 2048 x 192 x 192 6.2 against 7.9 (64x64 tiles)
    if (K % 64 == 0 && K % 128 != 0 && (long long)cdiv(M, 32) * cdiv(N, 64) <= 256) return 12;
    if (K % 64 == 0 && (long long)cdiv(M, 64) * cdiv(N, 64) >= 96) return 8;  // 64x64 tiles, KS 2, 3 stages
    return -1;
}

// Tile choice, from tools/gemm_tune.py on the benchmark's shapes:
// on this path K is short (192..2560), so a launch is dominated by how well the prologue /
// epilogue of one workgroup overlaps the MFMA loop of its neighbours.  Small wave tiles
// (32x32 per wave, 4-5 waves per SIMD) win almost everywhere; the 128x128 tile only pays
// when the output is large enough to fill every CU several times over.
//   cfg 0: 128x128, 8 waves (64x32 per wave)   cfg 5: 128x64, 8 waves (32x32 per wave)
//   cfg 2:  64x64,  4 waves (32x32 per wave)
int choose_cfg(const GemmArgs& a) {
    // N <= 32 with many rows (encoder_embed.conv.4 as an implicit GEMM: 632 736 x 32 x 72 at the headline shape): a 64-column tile
    // multiplies 32 columns of padding
    if (a.N <= 32 && a.M >= 4096) return 12;
    // (the third embed convolution, 307 040 x 128 x 288, stays on 128x64 with K steps of 32: one 128-column tile that gathers each A row once is
    // 301 against 284 us, K steps of 64 382)
    if (a.N <= 64) return 2;    // 64x64 tiles, 4 waves
    if (a.M <= 64) return 3;    // a handful of rows (per-frame recurrent products, batched over layers): 64x64 tiles, K step 64
    // few output tiles (streaming chunks: 256..2048 rows): the launch is one latency-bound K sweep per
    // workgroup; small tiles with a 64-deep K step are fastest (tools/gemm_tune.py on the streaming shapes)
    if ((long long)cdiv(a.M, 128) * cdiv(a.N, 64) * a.nb0 * a.nb1 < 144) return 3;  // fewer 128x64 tiles than ~half the CUs
    if (a.N <= 128 && a.M < 32768) return 3;   // 64x64 tiles, K step 64 (the ConvNeXt 1x1s have enough rows for 128x64)
    {   // N a multiple of 96 and a multi-round 128x64 grid that leaves the last round mostly empty: 64x96 tiles balance it
        // (measured -9 % on 4064x1152x512, -4 % on 2048x1536x768; no gain on single-round grids, which are bubble-bound)
        const long long b5 = (long long)cdiv(a.M, 128) * cdiv(a.N, 64), b6 = (long long)cdiv(a.M, 64) * (a.N / 96);
        const bool plain = a.cv_Fout == 0 && !a.w_kn && a.nb0 * a.nb1 == 1 && a.K % 32 == 0 && a.K >= 64;
        if (plain && a.N % 96 == 0 && b5 > 256 && cdiv(b6, 256) * 6144 * 100 <= cdiv(b5, 256) * 8192 * 80) return 11;
        // 128x64 tiles that fill the last round of the 256 CUs badly while 64x64 tiles fill it well (the 6.25 Hz stack: 2048 rows x
        // 1536 / 2080 / 2560 columns -> 384 / 528 / 640 tiles): the smaller tile costs ~7 % per tile and wins 7-14 % on balance
        // (tools/probes/m2048_probe.py)
        const long long b9 = (long long)cdiv(a.M, 64) * cdiv(a.N, 64);
        const double e5 = (double)b5 / (double)(cdiv(b5, 256) * 256), e9 = (double)b9 / (double)(cdiv(b9, 256) * 256);
        if (plain && a.K >= 512 && b5 > 256 && e9 >= e5 + 0.12) return 9;
    }
    return 5;                   // 128x64 tiles, 8 waves (LDS-DMA pipeline when K % 32 == 0)
}

}  // namespace

GemmForce decode_gemm_force(int code) {
    GemmForce f;
    if (code < 0) return f;
    if (code >= 3000) {         // 16x16x4 pipelined kernel table
        f.kind = GemmForce::P16;
        f.idx = code - 3000;
    } else if (code >= 2000) {  // pipelined kernel table
        f.kind = GemmForce::PIPE;
        f.idx = code - 2000;
    } else if (code >= 100) {   // ring kernel table
        f.kind = GemmForce::RING;
        f.idx = (code - 100) & 0xff;
        f.ablate = (code - 100) >> 8;
    } else {
        f.kind = GemmForce::CFG;
        f.idx = code & 0x3f;
        f.ablate = code >> 8;
        f.dma = !(code & 0x40);  // +64: classic (register-staged) kernel
    }
    return f;
}

void debug_force_gemm_cfg(int code) { g_force = decode_gemm_force(code); }
GemmForce gemm_force() { return g_force.kind != GemmForce::AUTO ? g_force : decode_gemm_force(tunables().gemm_cfg); }

GemmPlan plan_gemm(const GemmArgs& a, const GemmForce& f) {
    const int nb = a.nb0 * a.nb1;
    // what the LDS-DMA-fed kernels (LDS-DMA, ring, pipe, p16) have a form for: plain [N,K] operands, no mul / res_div / act_after_res
    const bool dma_form = a.cv_Fout == 0 && !a.w_kn && !a.mul && a.res_div == 1 && !a.act_after_res;
    GemmPlan p;
    switch (f.kind) {  // tuning hooks
        case GemmForce::P16:
            K2_REQUIRE(dma_form && !a.glu && a.K % 32 == 0 && a.K >= 64 && nb == 1, "p16 cfg %d does not fit this GEMM", f.idx);
            K2_REQUIRE(entry(GemmFamily::P16, f.idx, &p), "no p16 cfg %d", f.idx);
            return p;
        case GemmForce::PIPE:
            K2_REQUIRE(dma_form && a.K % 32 == 0 && a.K >= 64 && nb == 1, "pipe cfg %d does not fit this GEMM", f.idx);
            K2_REQUIRE(entry(GemmFamily::PIPE, f.idx, &p), "no pipe cfg %d", f.idx);
            return p;
        case GemmForce::RING: {
            K2_REQUIRE(entry(GemmFamily::RING, f.idx, &p), "no ring cfg %d", f.idx);
            const int ks = kRing[f.idx].KS;
            K2_REQUIRE(dma_form && a.K % (32 * ks) == 0 && a.K >= 32 * ks, "ring cfg %d does not fit this GEMM", f.idx);
            p.ablate = f.ablate;
            return p;
        }
        default: break;
    }
    const bool forced = f.kind == GemmForce::CFG;
    const int cfg = forced ? f.idx : choose_cfg(a);
    const bool plain = a.cv_Fout == 0 && !a.w_kn && nb == 1 && a.K % 64 == 0 && a.K >= 64;
    // (a) N <= 96: few columns; (b) small problems (streaming chunks, beam search: a 128x64 grid would leave most CUs idle and
    // every workgroup would walk K serially): the same kernel over column chunks of 96
    // (16-row workgroups re-read the weight chunk M/16 times: with many rows and a short K the 64x64 tiles are better)
    const bool few_tiles = (long long)cdiv(a.M, 128) * cdiv(a.N, 64) < 144 && a.M <= 4096 && !(a.M >= 2048 && a.K <= 256 && a.N > 272);
    const bool skinny_ok = !forced && plain && !a.mul && ((a.N <= 96 && a.M >= 512) || few_tiles);
    const bool skinny16_ok = skinny_ok && !a.glu;  // the 16-column C/D layout of gemm_f32_mfma_skinny has no lane pair 16 apart
    if (skinny_ok && few_tiles && a.N > 96 && a.res_div == 1 && !a.act_after_res) {
        const int ring = small_ring_entry(a.M, a.N, a.K);
        if (ring >= 0) return make(GemmFamily::RING, ring, f.ablate);
    }
    // a few hundred rows x <= 96 columns with a long enough K (the streaming value projections of the downsampled stacks: 256 x 96 x 512,
    // 512 x 48 x 384): 32x32 ring tiles with the K step split four ways, 6.4 / 5.7 against 9.3 / 6.5 us (same lab run)
    if (skinny16_ok && a.N <= 96 && a.M <= 512 && a.K % 128 == 0 && a.K >= 384 && a.res_div == 1 && !a.act_after_res)
        return make(GemmFamily::RING, 15, f.ablate);
    if (skinny16_ok) {
        if (a.N <= 48) return make(GemmFamily::SKINNY3, 0, f.ablate);
        if (a.K % 128 == 0 && ((a.K >= 1024 && (long long)cdiv(a.M, 16) * cdiv(a.N, 96) <= 384) ||
                               (a.K >= 512 && (long long)cdiv(a.M, 16) * cdiv(a.N, 96) <= 128)))
            return make(GemmFamily::SKINNY6_8, 0, f.ablate);
        return make(GemmFamily::SKINNY6, 0, f.ablate);
    }
    const bool dma_ok = dma_form && a.K % 32 == 0 && a.K >= 64 && a.lda % 4 == 0 && f.dma;
    if (dma_ok && !forced && nb > 1 && a.M <= 64) {
        // a handful of rows against many layers' weight matrices (LSTM wavefront): a weight-streaming problem -- 64x64 tiles, three
        // 16 KB stages in flight per workgroup
        // enough workgroups to keep ~3 per CU streaming (bytes in flight are what sets the rate): 32-column tiles when 64-column
        // tiles would give fewer than ~600
        return make(GemmFamily::DMA, (long long)cdiv(a.N, 64) * nb < 600 ? 20 : 21, f.ablate);
    }
    // One problem per launch, K % 32 == 0: the pipelined kernel, tile by a small cost model fitted to tools/gemm_lab.py offline.
    // The busiest CU runs ceil(tiles / 256) tiles; a tile costs its K steps plus a fixed part (prologue,
    // last steps, epilogue -- less of it is exposed when several small workgroups share the CU), small tiles pay a few percent
    // for their extra operand traffic.  Examples it reproduces: 4064 x 512 -> 128x64 (256 tiles, one round); 4064 x 1152,
    // 2048 x 2560 / 2080 -> 64x64 (1152 / 1280 / 1056 tiles: 4.5 / 5 / 4.1 rounds of 4096 instead of 2.25 / 2.5 / 2.1 -> 3 of 8192);
    // 4064 x 1024 / 1920, 2048 x 2048 -> 128x128; 16160 x 192 -> 64x64 or 128x32 (3 rounds of 4096 instead of 2 of 8192).
    if (dma_ok && !forced && nb == 1 && a.M >= 256 && (long long)a.M * a.lda < (1ll << 29) && (long long)a.N * a.ldw < (1ll << 29)) {
        struct Cand { int idx, bm, bn; double fixed_steps, penalty; };
        static const Cand cands[] = {{8, 128, 128, 3.5, 0.0}, {1, 128, 64, 3.3, 0.02}, {5, 64, 64, 4.0, 0.12}, {13, 128, 32, 5.5, 0.08}};
        const double nk = a.K / 32.0;
        int best = -1;
        double best_cost = 0;
        for (const Cand& c : cands) {
            const long long tiles = (long long)cdiv(a.M, c.bm) * cdiv(a.N, c.bn);
            const double cost = (double)cdiv(tiles, 256) * c.bm * c.bn * (nk + c.fixed_steps) * (1.0 + c.penalty);
            if (best < 0 || cost < best_cost) {
                best = c.idx;
                best_cost = cost;
            }
        }
        // The 16x16x4 form's 64 x 96 tile (gemm_f32_mfma_p16, round 5) where N is a multiple of 96 and the same model prefers it: the
        // launches that quantise badly in 32 x 32 blocks -- 2048 x 768 is 256 tiles of 64 x 96 against 192 of 128 x 64 (tools/gemm_lab.py,
        // round 5: 69.3 against 83.5 us at K = 2560, 57.2 / 67.8 at 2048, 44.7 / 52.5 at 1536, 25.7 / 29.0 at 768;
        // 4064 x 1152 x 512 47.4 / 48.3; it loses where 128 x 64 already divides the output: 8096 x 768 x 256 40.7 / 36.3, which the model
        // reproduces).  One wave per SIMD on a single-round grid, so its prologue and tail are fully exposed: six fixed steps.
        if (a.N % 96 == 0 && !a.glu && a.M >= 1024) {
            const long long tiles = (long long)cdiv(a.M, 64) * (a.N / 96);
            // (a long K loop amortises the form's extra operand traffic: 16160 x 192 x 2432 is 126.8 us on it against 134.8 on 128 x 32,
            // tools/gemm_lab.py, round 5 -- 6 % over the other tiles from 64 K steps, 10 % below)
            const double cost = (double)cdiv(tiles, 256) * 64 * 96 * (nk + 6.0) * (nk >= 64 ? 1.06 : 1.10);
            if (tiles >= 128 && cost < best_cost) return make(GemmFamily::P16, 0, f.ablate);
        }
        return make(GemmFamily::PIPE, best, f.ablate);
    }
    // (batched launches too -- the Conformer's per-(head, stream) score products -- as long as the tile choice is one of the DMA kernel's)
    if (dma_ok && (cfg == 5 || cfg == 0 || (cfg >= 7 && cfg <= 11))) return make(GemmFamily::DMA, cfg == 7 ? 5 : cfg, f.ablate);
    GemmPlan r = make(GemmFamily::REG, cfg == 7 || cfg == 8 || cfg == 11 ? 5 : (cfg <= 5 || cfg == 12) ? cfg : 2, f.ablate);
    r.mode = a.cv_Fout > 0 ? MODE_CONV : a.w_kn ? MODE_WKN : MODE_PLAIN;
    return r;
}

int gemm_kind(const GemmArgs& a, const GemmPlan& p) {
    const int base = a.cv_Fout > 0 ? 1 : (a.w_kn ? 2 : 0);
    switch (p.family) {
        case GemmFamily::REG: return base;
        case GemmFamily::DMA: return base + 16;
        case GemmFamily::SKINNY3: case GemmFamily::SKINNY6: case GemmFamily::SKINNY6_8: return base + 32;
        case GemmFamily::RING: return base + 64;
        // +128: a pipelined kernel, its tile in bits 8.. so that a profile can be grouped by instantiation: BM / 32, BN / 32; bit 20: 16x16x4
        case GemmFamily::PIPE: return base + 128 + 256 * (p.BM / 32) + 4096 * (p.BN / 32);
        case GemmFamily::P16: return base + 128 + 256 * (p.BM / 32) + 4096 * (p.BN / 32) + (1 << 20);
    }
    return base;
}

int glu_conv_ring_entry(int B, int Tc, int D, int K) {
    const int M = B * Tc, N = 2 * D;
    // tiles: 32 / 64 rows of whole streams (Tc | 32), 32 / 64 GEMM columns of whole (value | gate) blocks
    if (Tc < 2 || 32 % Tc != 0 || D % 64 != 0 || (K != 31 && K != 15 && K != 7)) return -1;
    // the K step split over the workgroup's wave groups as gemm() does for these shapes (streaming chunk steps: a few hundred tiles at
    // most); where gemm() would not take a ring tile, 64x64 tiles with KS 2 (entry 8)
    int e = small_ring_entry(M, N, D);
    if (e < 0) e = 8;
    // the tail's cache staging holds at most 8 elements per thread (conv_tail): tile's streams x channels x cached frames
    const RingCfg& r = kRing[e];
    if ((long long)(r.BM / Tc) * (r.BN / 2) * (K >> 1) > 8ll * (r.BM / 32) * (r.BN / 32) * r.KS * 64) return -1;
    return e;
}

// Offline conv module: in_proj + GLU + depthwise conv in one launch (gemm_glu_dwconv1d) where the GLU GEMM it replaces runs on a pipe
// tile that holds a whole stream.  The fused launch takes THAT tile -- so the in_proj sums, and with them the output, are those of the
// two launches bit for bit -- with one M tile per stream instead of M / BM packed ones.
int glu_dwconv_pipe_entry(int B, int T, int D, int K, bool streaming) {
    if (streaming || tunables().no_fused_conv || tunables().no_glu_epilogue) return -1;
    if (B < 1 || T < 1 || D < 1) return -1;
    const long long M = (long long)B * T;
    if (M < 256 || M * D >= (1ll << 29)) return -1;   // fewer rows: the engine runs the plain in_proj and the GLU in the conv kernel
    if (K != 15 && K != 31) return -1;                // the tail's instantiated tap counts (odd; its LDS strip has K - 1 halo rows)
    if (gemm_force().kind != GemmForce::AUTO) return -1;
    GemmArgs a;
    a.M = (int)M; a.N = 2 * D; a.K = D; a.lda = D; a.ldw = D; a.ldc = D; a.glu = 1;
    if (a.N <= 96 || a.N % 32 != 0) return -1;        // gemm()'s own conditions for the gated epilogue
    const GemmPlan p = plan_gemm(a, GemmForce());
    if (p.family != GemmFamily::PIPE || (p.idx != 1 && p.idx != 5 && p.idx != 8)) return -1;   // 128x64, 64x64, 128x128
    if (T > p.BM || a.N % p.BN != 0) return -1;       // a stream per tile; whole (value | gate) column tiles
    // one tile per stream must not add a round of the 256 CUs to the launch (T well below BM: half-empty tiles)
    const long long cols = a.N / p.BN;
    if (cdiv((long long)B * cols, 256ll) > cdiv((long long)cdiv(M, (long long)p.BM) * cols, 256ll)) return -1;
    return p.idx;
}

}  // namespace k2hip
