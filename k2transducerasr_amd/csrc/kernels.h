// Launchers for the gfx950 kernels.  Every launcher enqueues on ctx.stream and
// returns immediately; in a dry run (ctx.dry) nothing is launched -- the dry
// pass only sizes the arena.
#pragma once
#include "ctc_prefix_layout.h"
#include "common.h"

namespace k2hip {

// Switches of the library (tunables.cpp): the K2HIP_* environment read once at the first model creation.  The shipped build keeps
// ONE path per operation plus the cross-check pairs the parity tests compare (an alternative kernel for the same math, a forced
// fallback, a size limit); the tuning probes exist only in a -DK2HIP_DEV build (make DEV=1), where K2HIP_DEV_SWITCH fields become
// ordinary members -- here they are compile-time constants and the code behind them folds away.
#ifdef K2HIP_DEV
#define K2HIP_DEV_SWITCH(name, def) int name = def
#else
#define K2HIP_DEV_SWITCH(name, def) static constexpr int name = def
#endif
struct Tunables {
    // ---- cross-check pairs and forced fallbacks (tests/)
    int no_glu_epilogue = 0;      // K2HIP_NO_GLU_EPILOGUE: conv modules' GLU in the depthwise kernel instead of the in_proj GEMM's epilogue
    int attn_long = 0;            // K2HIP_ATTN_LONG: two-pass attention scores for every length (the long-utterance form)
    int no_fused_av = 0;          // K2HIP_NO_FUSED_AV: attention apply + out_proj as two GEMMs
    int fused_vproj_min_t = 4;    // K2HIP_FUSED_VPROJ_MIN_T: the streaming self-attention's value projection inside k_attn_av_out from this many
                                  // chunk rows per stream on (128 streams, device time per tick 3.61 ms from 4 rows on, 3.62 from 8, 3.68 from 2)
    int no_fused_vproj = 0;       // K2HIP_NO_FUSED_VPROJ: ... as a GEMM launch of its own
    int no_fused_conv = 0;        // K2HIP_NO_FUSED_CONV: the streaming conv modules' GLU + chunk-causal depthwise conv as a launch of its own
                                  // instead of inside the in_proj GEMM's epilogue (round 5)
                                  // (offline: the low-rate stacks' GLU GEMM + depthwise conv as two launches instead of gemm_glu_dwconv1d)
    int conformer_gemm_scores = 0;  // K2HIP_CONFORMER_GEMM_SCORES: two batched GEMMs + gather/softmax (the long-utterance form)
    int dw7_tiled = 0;            // K2HIP_DW7_TILED: the one-shot LDS-tiled 7x7 depthwise conv also for long inputs (default: the sliding LDS-DMA form)
    int dw1d_tt = 0;              // K2HIP_DW1D_TT: outputs per thread of the depthwise Conv1d (8 / 4 / 2; 0 = by grid size; tests/test_kernels_gpu.py forces each)
    int lstm_seq = 0;             // K2HIP_LSTM_SEQ: layer-by-layer LSTM instead of the layer wavefront
    int greedy_one_part = 0;      // K2HIP_GREEDY_ONE_PART: one workgroup per stream in the search
    int greedy_parts = 0;         // K2HIP_GREEDY_PARTS: vocabulary slabs per stream (0 = automatic)
    int beam_launches = 0;        // K2HIP_BEAM_LAUNCHES: the modified beam search as 4 launches per frame (the large-vocabulary form) even when the one-kernel form applies
    int beam_parts = 0;           // K2HIP_BEAM_PARTS: 1 = one workgroup per stream in the one-kernel beam search even where two column slabs apply
    int beam_hyp_global = 0;      // K2HIP_BEAM_HYP_GLOBAL: the one-kernel beam search keeps its hypotheses in device memory even when they fit in LDS (the long-utterance form)
    int beam_trace = 0;           // K2HIP_BEAM_TRACE: the modified beam search records its per-frame selection (k2hip_debug.h: k2hip_debug_beam_trace)
    int search_rounds = -1;       // K2HIP_SEARCH_ROUNDS: 1 = every multi-stream search as rounds of joiner GEMMs (greedy_rounds),
                                  // 0 = always the persistent kernel (k_greedy), -1 = measured default
    int test_greedy_timeout = 0;  // K2HIP_TEST_GREEDY_TIMEOUT: test hook -- every parts > 1 search reports an exchange timeout, so the one-part retry runs
                                  // (1: without arming the engine's back-off, so that the next search is parted again; 2: as a real one)
    // ---- limits
    int decoder_table_mb = 1024;  // K2HIP_DECODER_TABLE_MB: build the all-contexts decoder table when it fits this many MiB (0 = never)
    int screen_min_v = 1024;      // K2HIP_SCREEN_MIN_V: vocabularies of at least this size get the f16 screening pass in the greedy search
                                  // (greedy.hip screen_round: exact tokens, ~2.5x fewer bytes per round); 0 = never
    int screen_count = 0;         // K2HIP_SCREEN_COUNT: the persistent search counts, per round and part, whether the f16 screen decided the round or it
                                  // went to the f32 passes (k2hip_debug.h: k2hip_debug_op_run "greedy_screen_counts"); 0 = the kernel gets no counter
    int max_streams = 0;          // K2HIP_MAX_STREAMS: slots of the streaming state pool (0 = 256)
    int rnn_lm_gx_cap = 0;        // K2HIP_RNN_LM_GX_CAP: floats of a neural-LM call's input products per time block (0 = rnn_lm_plan.h's 2^26;
                                  // tests/test_rnn_lm_gpu.py forces a small one to take the time-blocked route)
    // ---- tuning probes (-DK2HIP_DEV builds only)
    K2HIP_DEV_SWITCH(gemm_cfg, -1);         // K2HIP_GEMM_CFG: force one tile configuration (a k2hip_debug_gemm cfg code: GemmForce)
    K2HIP_DEV_SWITCH(xcd_panels, 0);        // K2HIP_XCD_PANELS: 1 = every GEMM's tiles as bands of M per XCD (rounds 1 - 3)
    K2HIP_DEV_SWITCH(greedy_stamps, 0);     // K2HIP_GREEDY_STAMPS: the persistent search reports where a round's time goes (stderr, synchronous)
    K2HIP_DEV_SWITCH(conformer_stamps, 0);  // K2HIP_CONFORMER_STAMPS: the Conformer scores kernel reports its phases (stderr, synchronous)
};
void tunables_init_from_env();            // idempotent; called by k2hip_model_create
const Tunables& tunables();
bool tunables_set(const char* env_name, int value);  // test hook (k2hip_debug_set_switch)

struct GemmStats {
    double flops = 0;       // algorithmic, 2*M*N*K per launch
    double total_flops = 0; // + non-GEMM matrix work (attention scores, convs)
    int launches = 0;
    float ms = 0;           // summed event time (instrumented runs only)
};

struct GemmLaunchRec {  // one row per GEMM launch of an instrumented call
    int M, N, K, batch, act, res, kind;  // kind: 0 plain, 1 conv gather, 2 [K,N] operand; + the kernel family (gemm_kind)
    float us;
};

struct GreedyLaunch;
struct Ctx {
    std::vector<GemmLaunchRec>* gemm_log = nullptr;  // instrumented runs only
    GreedyLaunch* greedy_rec = nullptr;  // greedy_loop notes its launch here, so that the engine can repeat it with one part per stream
    hipStream_t stream = nullptr;
    Arena* arena = nullptr;
    bool dry = false;
    bool one_part = false;    // the engine's searches recently timed out waiting for their other column slabs (a GPU shared with other
                              // handles or processes): one workgroup per stream until the back-off runs out (Engine::note_search)
    bool instrument = false;  // bracket each GEMM launch with events
    GemmStats* stats = nullptr;
    // instrumented runs: each GEMM launch records a (start, stop) pair from this pool
    // WITHOUT synchronising; the engine reads the pairs after the call has drained,
    // so the launches run back to back exactly as in an un-instrumented call.
    std::vector<hipEvent_t>* evpool = nullptr;
    int* evused = nullptr;
    hipEvent_t next_event() const {
        if ((size_t)*evused == evpool->size()) {
            hipEvent_t e;
            K2_HIP(hipEventCreate(&e));
            evpool->push_back(e);
        }
        return (*evpool)[(*evused)++];
    }
    // algorithmic work is tallied once, in the dry (sizing) pass
    void add_flops(double gemm_fl, double other_fl, int launches) const {
        if (stats && dry) {  // stats may be null (tuning hook)
            stats->flops += gemm_fl;
            stats->total_flops += gemm_fl + other_fl;
            stats->launches += launches;
        }
    }
};

enum Act : int { ACT_NONE = 0, ACT_SWOOSH_L = 1, ACT_SWOOSH_R = 2, ACT_TANH = 3, ACT_SIGMOID = 4, ACT_RELU = 5, ACT_DOUBLE_SWISH = 6 };

// C[M,N] = act(A[M,K] . W^T + bias) (+ residual)     (fp32 MFMA, exact-f32 products)
//   A: row-major, K contiguous, lda % 4 == 0; rows may be gathered (implicit conv)
//   W: [N,K] row-major (torch Linear layout), or [K,N] when w_kn
struct GemmArgs {
    const float* A = nullptr;
    const float* W = nullptr;
    const float* bias = nullptr;
    const float* res = nullptr;
    float* C = nullptr;
    int M = 0, N = 0, K = 0;
    int lda = 0, ldw = 0, ldc = 0, ldr = 0;
    int act = ACT_NONE;
    int xcd_panels = 0;  // tile order: 0 = N panels per XCD chosen by PN M + (8 / PN) N (gemm.hip xcd_tile); 1 = a band of M per XCD (K2HIP_XCD_PANELS)
    int act_cols = 0;  // > 0: the activation applies to output columns < act_cols only (two Linears of one input fused in one launch)
    int w_kn = 0;
    // batching over blockIdx.z = z0 + nb0 * z1
    int nb0 = 1, nb1 = 1;
    // device flag: the launch does nothing when *skip_if_zero == 0 (rounds of the batched search after every stream has finished)
    const int* skip_if_zero = nullptr;
    long long sA0 = 0, sA1 = 0, sW0 = 0, sW1 = 0, sC0 = 0, sC1 = 0, sR0 = 0, sR1 = 0;
    long long sBias0 = 0;  // bias + z0 * sBias0 (batched launches over layers, each with its own bias)
    // implicit-conv gather of A over an NHWC tensor [B, Tin, Fin, C]:
    //   row r = (b*Tout + t)*Fout + f  ->  base = ((b*Tin + t*st)*Fin + f*sf)*C
    //   k -> (k / seg_len) * seg_stride + k % seg_len
    int cv_Fout = 0, cv_Tout = 0, cv_Tin = 0, cv_Fin = 0, cv_C = 0, cv_st = 1, cv_sf = 1;
    int seg_len = 0, seg_stride = 0;
    // epilogue extras (after bias, activation and residual):
    //   mul:  v *= mul[row*ldm + col]                      (batched like C: + z0*sM0 + z1*sM1)   -- NonlinAttention's output gate
    //   byp:  v = o + (v - o) * byp_scale[col], o = byp_orig[row*ld_orig + col]                 -- Zipformer bypass module
    //   res_div > 1: residual row = row / res_div (K hypothesis rows share their stream's encoder frame)
    //   act_after_res: v = act(acc + bias + res) instead of act(acc + bias) + res          -- the joiner's tanh(enc + dec)
    int res_div = 1;
    int act_after_res = 0;
    // glu: the N output columns are blocks of 32 = 16 values | their 16 gates (weights interleaved at load, "#glu"); the epilogue
    // writes value * sigmoid(gate) to N / 2 columns of C (ldc counts those).  32-column C/D layouts only (not the skinny kernel).
    int glu = 0;       // 1: value * sigmoid(gate) (conv modules), 2: value * tanh(gate) (NonlinAttention)
    int glu_cols = 0;  // > 0: only the first glu_cols GEMM columns are (value | gate) blocks; the rest pass through behind them
    const float* mul = nullptr;
    int ldm = 0;
    long long sM0 = 0, sM1 = 0;
    const float* byp_orig = nullptr;
    const float* byp_scale = nullptr;
    int ld_orig = 0;
    // Streaming conv module (round 5, gemm_glu_causal_conv below): the in_proj GEMM over "#glu"-interleaved weights finishes with the
    // GLU AND the chunk-causal depthwise convolution of online.hip's k_glu_causal_conv_reg -- the Tc rows of a stream sit in one tile, a
    // 32-column block holds 16 channels' values and gates, so everything the convolution of those channels needs is in the workgroup
    // (+ the stream's K / 2 cached frames from the state pool, which it also advances).  C = y [M, N / 2].
    float* cf_pool = nullptr;          // != nullptr: the fused form
    long long cf_stride = 0, cf_off = 0;
    const int* cf_slots = nullptr;
    const float *cf_wc = nullptr, *cf_bc = nullptr, *cf_ww = nullptr, *cf_bw = nullptr, *cf_sc = nullptr;
    int cf_Tc = 0, cf_K = 0;
    unsigned long long* dbg = nullptr;  // tuning only: in-kernel s_memtime stamps of the ring kernel, [workgroup][wave][64]
    int ablate = 0;  // tuning only: 1 = skip in-loop global loads, 2 = skip MFMAs, 4 = skip epilogue stores
    // Offline conv module (gemm_glu_dwconv1d below): the in_proj GEMM over "#glu"-interleaved weights finishes with the GLU AND the
    // depthwise Conv1d over time + bias + SwooshR of elementwise.hip's k_glu_dwconv1d<false, false> -- one M tile per stream (the tile of
    // stream b starts at row b dw_T, its rows >= dw_T are dead), so the tile that has just finished the GLU holds every frame the
    // convolution of its channels needs; zero rows in LDS are the time halo.  C = y [M, N / 2].  (Behind the tuning fields so that every
    // other launch keeps its argument layout.)
    const float* dw_w = nullptr;       // != nullptr: the fused form; taps [dw_K][N / 2] ("#kd")
    const float* dw_b = nullptr;       // conv bias [N / 2]
    int dw_K = 0, dw_T = 0;            // taps (15 or 31), frames per stream (<= the tile's BM)
};
void gemm(const Ctx& ctx, const GemmArgs& a);
// Conv module of a streaming Zipformer2 layer, first two thirds in ONE launch: y [M, D] = SwooshR(chunk-causal depthwise conv(GLU(x Wg^T + bg)))
// with the streams' conv caches (pool slot + off, [D][K / 2]) read and advanced in place; M = B Tc rows, stream-major.  wg / bg: the
// "#glu" row-interleaved in_proj [2 D, D]; wc / bc / ww / bw / sc: causal_conv, chunkwise_conv and chunkwise_conv_scale as
// glu_causal_conv takes them.  Returns false (nothing launched, nothing tallied) when the shape has no fused form -- the caller then
// runs linear + glu_causal_conv.  The convolution's sums are formed in k_glu_causal_conv_reg's order; the in_proj product in the order of
// this launch's tile form (the dispatcher's own choice for most of these shapes): equal to the two launches up to float rounding.
bool gemm_glu_causal_conv(const Ctx& ctx, const float* x, const float* wg, const float* bg, float* pool, long long slot_stride, long long off,
                          const int* slots, const float* wc, const float* bc, const float* ww, const float* bw, const float* sc, float* y, int B,
                          int Tc, int D, int K);

// Conv module of an offline Zipformer2 layer, first two thirds in ONE launch: y [B T, D] = SwooshR(depthwise conv_K(GLU(x Wg^T + bg)) + bd),
// zero-padded in time per stream.  wg / bg: the "#glu" row-interleaved in_proj [2 D, D]; wd: taps [K][D] ("#kd"); bd [D].  Returns
// false (nothing launched, nothing tallied) when glu_dwconv_pipe_entry has no fused form for the shape -- the caller then runs the GLU
// GEMM + dwconv1d_swoosh.  Same pipe tile as that GEMM, same sums in k_glu_dwconv1d's order: bit-identical to the two launches.
bool gemm_glu_dwconv1d(const Ctx& ctx, const float* x, const float* wg, const float* bg, const float* wd, const float* bd, float* y, int B, int T,
                       int D, int K);

// ---- GEMM tile plan (gemm_plan.cpp, host only): which kernel instantiation gemm() launches for a GemmArgs, decided without
// launching.  The tile tables of the kernel families; a table index is the k2hip_debug_gemm cfg code that forces the entry, less the
// family's base (pipe 2000, p16 3000, ring 100, LDS-DMA and register-staged 0).
// pipelined kernel on 32x32x2 MFMAs (gemm_f32_mfma_pipe): BM, BN, WM, WN, stages
#define K2_PIPE_TABLE(X)                                                                                                       \
    X(0, 128, 64, 64, 32, 3) X(1, 128, 64, 32, 32, 3) X(2, 128, 128, 64, 64, 3) X(3, 128, 128, 64, 32, 3) X(4, 128, 64, 64, 32, 4)  \
    X(5, 64, 64, 32, 32, 3) X(6, 128, 128, 64, 64, 4) X(7, 64, 128, 32, 64, 3) X(8, 128, 128, 32, 32, 3) X(9, 128, 64, 32, 32, 4) \
    X(10, 64, 64, 64, 32, 3) X(11, 64, 64, 32, 64, 3) X(12, 256, 64, 64, 32, 3) X(13, 128, 32, 32, 32, 3) X(14, 128, 32, 64, 32, 3)
// pipelined kernel on 16x16x4 MFMAs (gemm_f32_mfma_p16): 4 waves of 32 x 48, 64 x 48, 32 x 96, 16 x 48
#define K2_P16_TABLE(X) X(0, 64, 96, 32, 48, 3) X(1, 128, 96, 64, 48, 3) X(2, 64, 192, 32, 96, 3) X(3, 32, 96, 16, 48, 3)
// ring kernel (gemm_f32_mfma_ring): BM, BN, K groups, stages, loader waves, L2-prefetch wave
#define K2_RING_TABLE(X)                                                                                        \
    X(0, 128, 64, 1, 2, 0, 0) X(1, 128, 64, 1, 3, 0, 0) X(2, 128, 64, 1, 2, 0, 1) X(3, 128, 64, 1, 3, 0, 1) X(4, 128, 64, 1, 4, 0, 1)   \
    X(5, 64, 64, 1, 3, 0, 0) X(6, 64, 64, 1, 3, 0, 1) X(7, 64, 64, 1, 4, 0, 1) X(8, 64, 64, 2, 3, 0, 0) X(9, 64, 64, 2, 3, 0, 1)      \
    X(10, 64, 64, 4, 2, 0, 0) X(11, 64, 64, 4, 2, 0, 1) X(12, 32, 64, 2, 3, 0, 0) X(13, 32, 64, 4, 3, 0, 0) X(14, 32, 64, 4, 3, 0, 1)  \
    X(15, 32, 32, 4, 3, 0, 0) X(16, 32, 32, 4, 4, 0, 1) X(17, 64, 32, 4, 3, 0, 0) X(18, 128, 128, 1, 2, 0, 0) X(19, 128, 128, 1, 2, 0, 1) \
    X(20, 64, 128, 1, 3, 0, 0) X(21, 64, 128, 1, 3, 0, 1) X(22, 64, 96, 1, 3, 0, 0) X(23, 64, 96, 1, 3, 0, 1) X(24, 128, 96, 1, 2, 0, 1) \
    X(25, 128, 64, 1, 3, 2, 0) X(26, 128, 64, 1, 3, 2, 1) X(27, 128, 64, 2, 2, 0, 1) X(28, 64, 96, 2, 3, 0, 0) X(29, 64, 96, 2, 2, 0, 0) \
    X(30, 64, 96, 2, 2, 0, 1) X(31, 128, 96, 1, 3, 0, 0) X(32, 128, 96, 1, 3, 0, 1)
struct RingCfg { int BM, BN, KS, NST, LW, PF; };
#define X(i, bm, bn, ks, nst, lw, pf) {bm, bn, ks, nst, lw, pf},
constexpr RingCfg kRing[] = {K2_RING_TABLE(X)};
#undef X
// LDS-DMA kernel (gemm_f32_mfma_dma): BM, BN, WM, WN, stages.  cfg 7 forces 5's tile; 20 and 21 are the batched few-row tiles, which
// no cfg forces.
#define K2_DMA_TABLE(X)                                                                                                          \
    X(0, 128, 128, 64, 32, 3) X(5, 128, 64, 32, 32, 2) X(8, 128, 64, 32, 32, 4) X(9, 64, 64, 32, 32, 2) X(10, 64, 64, 32, 32, 3) \
    X(11, 64, 96, 32, 32, 2) X(20, 32, 32, 32, 32, 4) X(21, 32, 64, 32, 32, 4)
// register-staged kernel (gemm_f32_mfma): BM, BN, WM, WN, BK.  cfg 7, 8, 11 force 5's tile, every other cfg below 64 2's.
#define K2_REG_TABLE(X)                                                                                                           \
    X(0, 128, 128, 64, 32, 32) X(1, 128, 128, 64, 32, 64) X(2, 64, 64, 32, 32, 32) X(3, 64, 64, 32, 32, 64) X(4, 128, 64, 32, 32, 64) \
    X(5, 128, 64, 32, 32, 32) X(12, 128, 32, 32, 32, 32)
enum GemmMode { MODE_PLAIN = 0, MODE_CONV = 1, MODE_WKN = 2 };  // the register-staged kernel's A / W addressing

// skinny: gemm_f32_mfma_skinny<3>, <6>, <6, 8> (16 rows x 48 / 96 columns per workgroup, 4 / 4 / 8 waves)
enum class GemmFamily { REG, DMA, PIPE, P16, RING, SKINNY3, SKINNY6, SKINNY6_8 };
struct GemmPlan {
    GemmFamily family = GemmFamily::REG;
    int idx = 0;                    // entry of the family's table (skinny: 0)
    int mode = MODE_PLAIN;          // REG only
    int ablate = 0;                 // GemmArgs.ablate (tuning only)
    int BM = 0, BN = 0, waves = 0;  // the entry's workgroup tile and waves per workgroup
};
// A forced tile choice (tuning hooks), decoded from a k2hip_debug_gemm cfg code by decode_gemm_force:
//   < 0: automatic
//   0 .. 63: the LDS-DMA tile of cfg (0, 5, 7 .. 11) where the GEMM suits that kernel, else the register-staged tile of cfg;
//            +64: register-staged only; +256 n: ablate n
//   100 + i (+256 n): ring entry i (ablate n);  2000 + i: pipe entry i;  3000 + i: p16 entry i
struct GemmForce {
    enum Kind { AUTO, CFG, RING, PIPE, P16 } kind = AUTO;
    int idx = -1;
    int ablate = 0;
    bool dma = true;  // CFG: the LDS-DMA kernel where the cfg names one of its tiles
};
GemmForce decode_gemm_force(int code);
// gemm()'s choice of kernel for a GEMM under a force; throws (K2HIP_ERR_INVALID) when a forced entry does not exist or does not fit
GemmPlan plan_gemm(const GemmArgs& a, const GemmForce& f);
int gemm_kind(const GemmArgs& a, const GemmPlan& p);  // GemmLaunchRec.kind of the launch
// the ring entry of gemm_glu_causal_conv's fused form for B streams of Tc rows and D channels, conv kernel size K; -1 = no fused form
int glu_conv_ring_entry(int B, int Tc, int D, int K);
// the pipe table entry (1: 128x64, 5: 64x64, 8: 128x128) of gemm_glu_dwconv1d's fused form for B streams of T frames, D channels and K
// taps; -1 = no fused form (streaming: the call comes from a streaming site, which has gemm_glu_causal_conv instead)
int glu_dwconv_pipe_entry(int B, int T, int D, int K, bool streaming);
void debug_force_gemm_cfg(int code);  // tuning hook: -1 = automatic
GemmForce gemm_force();  // what gemm() plans under: the tuning hook's force, else K2HIP_GEMM_CFG (DEV builds)
struct GemmForceGuard {  // forces cfg code `code` for its lifetime, automatic again on scope exit
    explicit GemmForceGuard(int code) { debug_force_gemm_cfg(code); }
    ~GemmForceGuard() { debug_force_gemm_cfg(-1); }
    GemmForceGuard(const GemmForceGuard&) = delete;
    GemmForceGuard& operator=(const GemmForceGuard&) = delete;
};
// convenience: plain Linear  C = act(A W^T + b) (+res)
void linear(const Ctx& ctx, const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int M, int K,
            int N, int act = ACT_NONE, const float* res = nullptr, int ldr = 0);

// A per-stream cache kept as a RING of KL = L + Tc rows inside the stream's slot of the state pool (streaming Zipformer2): the
// chunk's Tc new rows overwrite the Tc oldest ones in place, nothing is rolled.  Chunk n of a stream writes its row r to ring row
// (head + r) % KL, head = (n * Tc) % KL; in the order of the reference's [cache ; chunk] concatenation (j = 0 oldest .. KL - 1
// newest) row j is at (head + Tc + j) % KL.
struct RingRef {
    float* pool = nullptr;         // state pool
    long long slot_stride = 0;     // floats per stream
    long long off = 0;             // float offset of this ring inside a slot
    const int* slots = nullptr;    // [B] slot of each stream of the step
    const int* chunks = nullptr;   // [B] chunks each stream has decoded before this step
};

// ---- attention ------------------------------------------------------------
// qkp: [B*T, ld] rows = (q[H*32] | k[H*32] | p[H*4]); pp: [2T-1, H*4];
// aw out: [H][B][T][Tp] (Tp = T rounded up to 4, pad columns zeroed)
// qh: query / key head size (16, 24 or 32); koff0 / poff0: float offset of head 0's key / positional query in a row (default: the
// Zipformer2 row above; Zipformer v1: q [A] | k [A] | v [A/2] | p [H*4])
void attn_scores_softmax(const Ctx& ctx, const float* qkp, int ld, const float* pp, float* aw, int B, int T, int Tp, int H, int qh = 32,
                         int koff0 = -1, int poff0 = -1);

// fused x += out_proj(concat_h(aw_h . v_h)) + bias  (SelfAttention after its value projection); aw [H][B][T][Tp] over KL keys,
// v [B*KL, H*vh], wout [D, H*vh];
// returns false (nothing launched, nothing tallied) when the shape does not fit the kernel -- the caller then takes the GEMM path
bool attn_av_out(const Ctx& ctx, const float* aw, const float* v, const float* wout, const float* bias, float* x, int B, int T, int KL, int Tp,
                 int H, int vh, int D);
// streaming ring form: values of the left context come from the ring (rows in ring order, like aw's columns); the chunk's value
// rows (newrows [B*T, H*vh]) are written into the ring by the kernel itself before it reads them.  T <= 16 (one row strip).
bool attn_av_out_ring(const Ctx& ctx, const float* aw, const RingRef& vals, const float* newrows, const float* wout, const float* bias, float* x,
                      int B, int T, int KL, int Tp, int H, int vh, int D);
void attn_proj_av_out_ring(const Ctx& ctx, const float* aw, const RingRef& vals, const float* xin, const float* win, const float* bin,
                           const float* wout, const float* bias, float* xout, int B, int T, int KL, int Tp, int H, int vh, int D);

// NonlinAttention.streaming_forward after its in_proj: hid [B*T, ldh] rows = s | x | y (Hc columns each); x * tanh(s) of the chunk's
// rows goes into the cache ring, then ctx = (aw_head0 . ring) * y.  wout != nullptr: x[B*T, D] += out_proj(ctx) in the same launch
// (every stream's workgroup pulls the whole out_proj matrix through its CU: only worth it for narrow stacks); wout == nullptr:
// x [B*T, Hc] = ctx, and the caller runs out_proj as a GEMM over all streams' rows.  T <= 16.
void nonlin_av_out_ring(const Ctx& ctx, const float* aw, const RingRef& cache, const float* hid, int ldh, const float* wout, const float* bias,
                        float* x, int B, int T, int KL, int Tp, int Hc, int D);

// ---- elementwise / small -----------------------------------------------------
// packed: all streams' features back to back; d_off/d_len: per-stream start and float count (device)
void pad_logfloor(const Ctx& ctx, const float* packed, const long long* d_off, const long long* d_len, float* out, int B,
                  long long L);
void pad_logfloor_dense(const Ctx& ctx, const float* feats, long long n_each, float* out, int B, long long L);
void conv0_swoosh(const Ctx& ctx, const float* x, const float* w, const float* b, float* y, int B, int T, int F);
// SwooshL (act 1) / SwooshR (act 2) of x[0 .. n) in the epilogues' lean form and in the library-log form it replaced (act.h), for
// the bit comparison of the two
void act_forms(const Ctx& ctx, const float* x, float* y_lean, float* y_libm, int act, long long n);
// Conformer Conv2dSubsampling conv.0: 1->8 ch, 3x3, padding 1 in time and frequency, DoubleSwish; y: NHWC [B,T,F,8]
void conv0_pad1_dswish(const Ctx& ctx, const float* x, const float* w, const float* b, float* y, int B, int T, int F);
// depthwise 7x7 over [B,Tin,F,C] -> [B,Tout,F,C]; time taps read in[t + kt - tpad] (zero outside [0,Tin)).
// offline ConvNeXt: Tin = Tout, tpad = 3; streaming: Tin = Tout + 6, tpad = 0 (left cache + right context supply the taps)
void dwconv7x7(const Ctx& ctx, const float* x, const float* w_kc, const float* b, float* y, int B, int Tin, int Tout, int tpad,
               int F, int C);
void biasnorm(const Ctx& ctx, const float* x, const float* bias, const float* log_scale, float* y, int M, int D);
// y = orig + (biasnorm(x) - orig) * scale     (layer tail: norm + bypass)
void biasnorm_bypass(const Ctx& ctx, const float* x, const float* orig, const float* nbias, const float* log_scale,
                     const float* scale, float* y, int M, int D);
// the same for the last layer of an input-rate stack in front of a downsampled one, and that stack's SimpleDownsample of the result
// (xd2 [B * ceil(T / ds2), D2]) in the same launch
void biasnorm_bypass_downsample(const Ctx& ctx, const float* x, const float* orig, const float* nbias, const float* log_scale, const float* scale,
                                float* y, const float* bias2, float* xd2, int B, int T, int D, int ds2, int D2);
// what a layer's last launch also has to produce when it is that layer (null bias2: nothing)
struct LayerTail {
    const float* bias2 = nullptr;
    float* xd2 = nullptr;
    int ds2 = 1, D2 = 0;
};
void bypass(const Ctx& ctx, const float* orig, const float* x, const float* scale, float* y, int M, int D);
void glu_sigmoid(const Ctx& ctx, const float* x, float* y, int M, int D);          // y = x[:, :D] * sigmoid(x[:, D:])
void tanh_gate(const Ctx& ctx, const float* x, float* y, int M, int Hc);           // y = x[:, Hc:2Hc] * tanh(x[:, :Hc])
// y = SwooshR(dwconv1d(glu(x2)) + b);  x2: [B,T,2D] value|gate
// the same on an input whose GLU has already run (x: [B,T,D]): GemmArgs.glu
void dwconv1d_swoosh(const Ctx& ctx, const float* x, const float* w_kd, const float* b, float* y, int B, int T, int D, int K);
void glu_dwconv1d_swoosh(const Ctx& ctx, const float* x2, const float* w_kd, const float* b, float* y, int B, int T, int D,
                          int K);
// same with DoubleSwish (Conformer ConvolutionModule)
void glu_dwconv1d_dswish(const Ctx& ctx, const float* x2, const float* w_kd, const float* b, float* y, int B, int T, int D,
                          int K);
// LSTM transducer (lstm.hip)
void conv0_nopad_dswish(const Ctx& ctx, const float* x, const float* w, const float* b, float* y, int B, int T, int F);
// gates i,f,g,o = gx[b] + gh[b] ([4*Hh] each, row strides ldgx / ldgh): c = f*c + i*g; hf = o * tanh(c)
void lstm_cell(const Ctx& ctx, const float* gx, long long ldgx, const float* gh, int ldgh, float* c, float* hf, int B, int Hh);
void add_inplace(const Ctx& ctx, float* a, const float* b, long long n);
// layer-wavefront form (lstm_engine.cpp): rows r = z*B + b over the n active layers z (layer lo + z works on frame s - lo - z)
//   gates [n*B, 4Hh] (both biases already added by the GEMMs) -> c [n*B, Hh] updated, hf [n*B, Hh]
void lstm_cell_rows(const Ctx& ctx, const float* gates, float* c, float* hf, int rows, int Hh);
//   h[z][b] = sum_q hp[q][z][b] (the S split-K partials of the projection, `pstride` floats apart); x1[z][b] = Y[lo+z][b*T + t_z] + h
//   (Y: [L+1][B*T][D], layer stride SY)
void lstm_add_frame(const Ctx& ctx, const float* Y, long long SY, const float* hp, long long pstride, int S, float* h, float* x1, int n, int B,
                    int T, int D, int lo, int s);
//   x2 = x1 + b2 + sum_q fp[q] (split-K partials of feed_forward.4); Y[lo+z+1][b*T + t_z] = BasicNorm(x2); b2 / eps of layer l at
//   b2_0 + l*lstride / eps0 + l*lstride
void lstm_norm_frame(const Ctx& ctx, const float* x1, const float* fp, long long pstride, int S, const float* b2_0, const float* eps0,
                     long long lstride, float* Y, long long SY, int n, int B, int T, int D, int lo, int s);
// rows of `width` floats between a [B, width] work buffer and the per-stream pool slots (pool + slot*stride + off)
void gather_rows(const Ctx& ctx, const float* pool, long long slot_stride, long long off, const int* slots, float* out, int B, int width);
void scatter_rows(const Ctx& ctx, float* pool, long long slot_stride, long long off, const int* slots, const float* in, int ldin, int B, int width);
// BasicNorm: y = x * (mean(x^2) + exp(log_eps))^-0.5   (in place allowed)
void basicnorm(const Ctx& ctx, const float* x, const float* log_eps, float* y, int M, int D);
// Conformer rel-pos attention helpers (conformer.hip)
//   qkv [M, 3D] -> qu = q*dk^-0.5 + pos_bias_u, qv = q*dk^-0.5 + pos_bias_v   ([M, D] each)
void conformer_qprep(const Ctx& ctx, const float* qkv, const float* bias_u, const float* bias_v, float* qu, float* qv, int M,
                     int D, float scaling, int ldq = 0 /* row stride of q; 0 = 3*D */);
// streaming (OnlineProjOfConformer): keys = [left cache ; chunk]; w[i,j] = softmax_j(ac[i,j] + bd[i, Tc-1-i+j]) over KL = left + Tc keys,
// left slot j masked (-inf) while plen[b] <= left-1-j; rows of stream b are z = b*H + h
void conformer_softmax_shift_stream(const Ctx& ctx, float* ac, const float* bd, const long long* plen, int B, int H, int Tc, int left,
                                    int KLp, int NPp);
void slice_rows(const Ctx& ctx, const float* in, float* out, int B, int Tin, int row0, int Tout, int D);  // out[b] = in[b][row0 : row0+Tout]
// y[b,t,:] = DoubleSwish(bias + sum_k w_kd[k] * cat[b, t+k, :])  (valid depthwise conv over [K-1 cached ; chunk] frames)
void dwconv_valid_dswish(const Ctx& ctx, const float* cat, const float* w_kd, const float* bias, float* y, int B, int Tc, int D, int K);
//   ac[z][i][j] (ld Tp) <- softmax_j(ac[z][i][j] + bd[z][i][T-1-i+j]) (rel_shift in gather form); pad columns zeroed
void conformer_softmax_shift(const Ctx& ctx, float* ac, const float* bd, int Z, int T, int Tp, int NPp);
// fused form: aw[b*H+h][i][:] = softmax_j((q+u)_i.k_j + (q+v)_i.p[T-1-i+j]) straight from qu / qv [B*T, D], k rows (row stride ldk) and the
// projected positional table pp [2T-1, D]; false = shape not covered (caller takes the GEMM + conformer_softmax_shift form)
bool conformer_scores_softmax(const Ctx& ctx, const float* qu, const float* qv, const float* kmat, int ldk, const float* pp, float* aw, int B, int H,
                              int T, int Tp, int D, int ldq = 0, const float* bias_u = nullptr, const float* bias_v = nullptr, float scaling = 1.0f);
// Din / Dorig > 0: the input rows are that wide and are zero-extended / truncated to D on the fly (convert_channels folded in)
void downsample(const Ctx& ctx, const float* x, const float* bias, float* y, int B, int T, int D, int ds, int Din = 0);
void upsample_combine(const Ctx& ctx, const float* orig, const float* xd, const float* scale, float* y, int B, int T,
                      int Td, int D, int ds, int Dorig = 0);
// the same and the NEXT stack's downsample of its result in one launch: y as above, xd2[b, t2, :D2] = sum_k softmax(bias2)_k y[b, ds2 t2 + k, :]
void upsample_combine_downsample(const Ctx& ctx, const float* orig, const float* xd, const float* scale, float* y, const float* bias2,
                                 float* xd2, int B, int T, int Td, int D, int ds, int Dorig, int D2, int ds2);
void convert_channels(const Ctx& ctx, const float* x, float* y, int M, int Din, int Dout);
// Zipformer2._get_full_dim_output without the concatenated tensor: columns [col1[i-1], col1[i]) of the full-width row live in src[i]
// (row width ld[i]); downsample_full = that gather + SimpleDownsample(ds) in one launch
struct FullDimSegs {
    const float* src[8];
    int ld[8], col1[8], n = 0;
    // segment 0 (the last stack's output) formed on the fly instead of read, when that stack is downsampled: its out_combiner
    // orig + (upsample(xd) - orig) * scale (k_upsample_combine's expression) -- the tensor itself is never written
    const float* lz_orig = nullptr;   // [B*T, lz_Do] (zero-extended / truncated to the stack's width)
    const float* lz_xd = nullptr;     // [B*lz_Td, ld[0]]
    const float* lz_scale = nullptr;
    int lz_Td = 0, lz_ds = 1, lz_Do = 0;
};
void downsample_full(const Ctx& ctx, const FullDimSegs& segs, const float* bias, float* y, int B, int T, int D, int ds);
void copy_cols(const Ctx& ctx, const float* x, int ldx, int xcol0, float* y, int ldy, int ycol0, int M, int n);

// ---- fbank -----------------------------------------------------------------------
struct FbankArgs {
    const float* samples;  // device
    long long n_samples;   // per utterance
    long long utt_stride;  // samples between utterances
    int n_utts;
    long long n_frames;    // per utterance
    float* feats;          // [n_utts, n_frames, 80]
    const float* window;
    const float* melw;
    int frame_len, frame_shift;
    float preemph, input_scale;
    int remove_dc;
    const float* melrange = nullptr;  // [num_bins][2] extent of each mel filter's non-zero weights (model table)
};
void fbank(const Ctx& ctx, const FbankArgs& a);
// dst[b][0 .. nmax) = src[b][0 .. n[b]) followed by zeros; src[b] may be pinned host memory (read in place over PCIe), 16 B aligned
void gather_samples(const Ctx& ctx, const float* const* src, const long long* n, float* dst, int B, long long nmax);

// ---- sample-rate conversion (resample.hip; the plan: resample_plan.h, the host reference: resample_ref.h) -------------------------
// One row of a resample_gather launch.  Its input is two pieces [head ; tail] (the carried tail of a stream and its new samples, or
// either alone), device memory or pinned host memory read in place.  w == nullptr: a pass-through row, dst row = the n_head + n_tail
// samples followed by zeros, as gather_samples moves them.  Otherwise outputs k0 .. k0 + n_out of the plan, followed by zeros;
// head[0] is input sample x0 of the stream, and samples in front of input sample 0 read as zero.
struct ResampleRow {
    const float* head = nullptr;
    const float* tail = nullptr;
    long long n_head = 0, n_tail = 0;
    long long x0 = 0, k0 = 0, n_out = 0;
    long long wmax = 0;                 // the plan's window in ticks: the launcher checks every row's reads against its input with it
    const float* w = nullptr;           // device: [ou][max_taps]
    const int* first = nullptr;         // device: [ou]
    const int* ntaps = nullptr;         // device: [ou]
    int iu = 0, ou = 0, max_taps = 0;
    int dst_row = 0;
};
constexpr int kResampleTile = 1024;     // outputs per workgroup trip at most (fewer when the ratio iu / ou is large: the span is staged in LDS)
// rows: B descriptors in host memory (checked here: no row reads outside its two pieces or writes outside its dst row), d_rows: the
// same B descriptors in device memory.  dst [n_dst_rows][nmax].
void resample_gather(const Ctx& ctx, const ResampleRow* rows, const ResampleRow* d_rows, int B, float* dst, int n_dst_rows, long long nmax);

// ---- voice activity detection (vad.hip; the definition and the host reference: vad_ref.h) -------------------------------------------
constexpr int kVadMaxW = 1024;   // floor_window at most (= vad_ref.h kVadMaxWindow)
constexpr int kVadTile = 256;    // frames per workgroup of the floor pass
// words of one stream's carried block: [W - 1 floats of m, right-aligned: the newest last | 4 floats of s | trig, start, te, segments
// emitted by the call (ints)]
inline long long vad_state_words(int W) { return (long long)W + 7; }
// One stream of a vad_run call: n > 0 feature rows (device; `stride` floats apart), row 0 being frame t0 of the stream.
struct VadRow {
    const float* feats = nullptr;
    long long stride = 0;
    int n = 0, t0 = 0, n_hist = 0;       // n_hist = min(t0, W - 1) values of m are carried
    int lo = 0, hi = 0, W = 0;
    float inv_band = 0.f, rise = 0.f, margin = 0.f, abs_floor = 0.f;
    int min_silence = 0, min_speech = 0, max_speech = 0;
    int trig = 0, start = 0, te = -1;    // the machine as the call finds it
    long long work_off = 0;              // the stream's first entry in s / m / n / d
    long long state_off = 0;             // ... word in st_in / st_out
    long long seg_off = 0;               // ... segment in segs [.][3] = (a, b, forced); at most seg_cap are written
    int seg_cap = 0;
};
struct VadBuffers {
    const float* st_in = nullptr;        // device: the carried blocks
    float* st_out = nullptr;             // device: the new ones, same layout
    float *s = nullptr, *m = nullptr, *n = nullptr;
    unsigned char* d = nullptr;
    int* segs = nullptr;
    long long n_work = 0, n_state = 0, n_segs = 0;   // entries of s / m / n / d, words of st_in / st_out, segments of segs
};
// rows: B descriptors in host memory (checked here before anything is launched: no stream reads or writes outside its extents),
// d_rows: the same in device memory
void vad_run(const Ctx& ctx, const VadRow* rows, const VadRow* d_rows, int B, const VadBuffers& buf);

// ---- neural LM rescoring (rnn_lm.hip; the definition and the host reference: rnn_lm_ref.h; the row layout: rnn_lm_plan.h) -----------
// The LM resident on the device, one allocation: the embedding [V][E]; per layer W_ih [4H][in] (torch layout: the GEMM launcher's), the
// summed bias [4H] and W_hh re-laid k-major as [H][4H] (whh_kn[k][g H + j] = W_hh[g H + j][k]: a half-wave's B operand of one k row
// is 128 contiguous bytes); the output matrix k-major [H][Vp], Vp = V rounded up to 32 with zero columns, and its bias [V].
struct RnnLmDev {
    int V = 0, Vp = 0, E = 0, H = 0, L = 0, sos = 0, eos = 0;
    const float* emb = nullptr;
    const float* w_ih[8] = {};
    const float* bias[8] = {};
    const float* whh_kn[8] = {};
    const float* out_kn = nullptr;
    const float* out_b = nullptr;
    // shallow fusion (rnn_lm_fuse.hip): per layer [W_ih ; W_hh] concatenated along k and re-laid in panels -- panel jb holds the four
    // gates of the 8 hidden columns 8 jb .. (column c = gate c / 8 of hidden column 8 jb + c % 8) over all k as [Kc / 4][32][4], Kc =
    // in rounded up to 32 (zero rows) + H, so a lane's B operand of
    // four consecutive k is ONE 16-byte load and a wave's load is 1 KiB contiguous; the output matrix once more in torch layout [V][H]
    // for the GEMM launcher; the start hypothesis' state after sos h0 / c0 [L][H] and its row q0 [V], computed on the device at upload;
    // work [2]: debug counters of k_nlm_advance launches that swept their weights / that only moved state
    const float* wcat[8] = {};
    const float* w_out = nullptr;
    float* h0 = nullptr;
    float* c0 = nullptr;
    float* q0 = nullptr;
    long long* work = nullptr;
};
// x0 [R][E] = emb[ids[row]]; ids in [0, V) (the caller's check)
void rnn_lm_embed(const Ctx& ctx, const float* emb, const int* ids, float* x0, long long R, int E);
// One position of one layer for the a active rows (a contiguous prefix): gates = gx[row] + h_prev[row] . W_hh^T on the matrix pipe
// (k ascending in one accumulator chain per output), the cell applied in the epilogue, c [a][H] updated in place, h stored into
// h_out [a][H].  gx rows are 4 H floats.  h_prev == nullptr: the first position (h = 0, the product is skipped).  Rows >= a of c and
// h_out are not touched; gates never reach memory.
void rnn_lm_step(const Ctx& ctx, const float* h_prev, const float* whh_kn, const float* gx, float* c, float* h_out, int a, int H);
// lp [R] = log_softmax(y[row] . W_out^T + b)[target[row]]: strips of 32 rows against out_kn with an online log-sum-exp, the logits never
// stored; columns >= V never enter the sum
void rnn_lm_score_rows(const Ctx& ctx, const float* y, const float* out_kn, const float* out_b, const int* target, float* lp, long long R, int H,
                       int V, int Vp);
// ---- neural LM shallow fusion in the modified beam search (rnn_lm_fuse.hip; semantics: include/k2hip.h "Neural LM shallow fusion") ----
// One layer of one frame over all M hypothesis slots.  Slot m continues slot par[m] of the other parity and appended tok[m] (-1: nothing).
// Rows that appended: gates = [x ; h_par[par[m]]] . wcat^T + bias on the matrix pipe (x = emb[tok[m]] when emb is set, else x_rows[m]),
// the cell in the epilogue against c_par[par[m]], h_out[m] / c_out[m] written; gates never reach memory.  Rows that appended nothing:
// h_out[m] = h_par[par[m]], c_out[m] = c_par[par[m]], bit for bit.  A workgroup owns 8 hidden columns x four gates and walks every
// 32-row strip of up to 256 rows against each weight it loads ONCE; strips without an appended row issue no matrix work, and with
// *live == 0 (null: live) the launch reads no weight at all.  in % 4 == 0, H % 32 == 0; par in [0, M), tok in [-1, V): the caller's.
struct NlmAdvance {
    const float* wcat = nullptr;    // the layer's panels (RnnLmDev::wcat)
    const float* bias = nullptr;    // [4H]
    const float* emb = nullptr;     // [V][in] (layer 0) or null
    const float* x_rows = nullptr;  // [M][in] (the layer below's new h) when emb is null
    const float* h_par = nullptr;   // [M][H] frame t's state of this layer
    const float* c_par = nullptr;
    float* h_out = nullptr;         // [M][H] frame t + 1's
    float* c_out = nullptr;
    const int* par = nullptr;       // [M]
    const int* tok = nullptr;       // [M]
    const int* live = nullptr;      // device flag or null
    long long* work = nullptr;      // debug counters or null (RnnLmDev::work)
    int M = 0, in = 0, H = 0;
};
void nlm_advance(const Ctx& ctx, const NlmAdvance& a);
// The LM rows of frame t + 1: q_out[m] = log_softmax(h[m] . W_out^T + b_out) over V for the slots that appended (the GEMM launcher,
// skipped on the device when *live == 0, then one workgroup per row), q_out[m] = q_par[par[m]] for the others.  Rows are V floats.
void nlm_rows(const Ctx& ctx, const float* h, const float* w_out, const float* out_b, const float* q_par, float* q_out, const int* par,
              const int* tok, const int* live, int M, int H, int V);
// The fused search's view of the LM (BeamArgs::nlm): dev.emb == null: off
struct BeamNlm {
    RnnLmDev dev;
    float scale = 0.f;
};
// the start state h0 / c0 and row q0 into every slot of parity 0: h, c [L][M][H], q [M][V]
void nlm_broadcast(const Ctx& ctx, const RnnLmDev& d, float* h, float* c, float* q, int M);
// The streaming (resumed) form: every stream of the call owns a device block (rnn_lm_stream_pool.h NlmStreamLayout{K, L, H, V}) that
// carries its slots' states and rows from chunk to chunk.  io [B] (device): per stream the half this call reads (null: a stream without
// a state yet) and the half it writes.
struct NlmStreamIO {
    const float* rd = nullptr;
    float* wr = nullptr;
};
// once per call, in place of nlm_broadcast: stream b's current half into slots b K .. b K + K - 1 of the parity-0 arrays h, c [L][M][H],
// q [M][V] (M = B K).  A stream with rd == null and every dead slot (k >= nh[b * nh_stride], the in blocks' first int) get the start
// state h0 / c0 / q0, so no LM launch reads undefined memory.  16 bytes per lane where both sides are aligned, floats elsewhere.
void nlm_load_streams(const Ctx& ctx, const RnnLmDev& d, const NlmStreamIO* io, const int* nh, int nh_stride, float* h, float* c, float* q, int B, int K);
// once per call, behind the last frame's LM launches: slots b K + k of the final-parity arrays into slot k of stream b's other half
void nlm_store_streams(const Ctx& ctx, const RnnLmDev& d, const NlmStreamIO* io, const float* h, const float* c, const float* q, int B, int K);
// h0 / c0 / q0 of d from h = c = 0 and sos, through the kernels above (once per upload)
void nlm_start_state(const Ctx& ctx, const RnnLmDev& d);
// launches of the fused search since the process started (the third counter beside beam_launch_counts)
void nlm_note_search();
long long beam_nlm_launch_count();
// ... and of the fused RESUMED search (chunk calls; k2hip_debug_rnn_lm_stream_fusion_stats), a counter of its own
void nlm_note_stream_search();
long long beam_nlm_stream_launch_count();

// One hypothesis of rnn_lm_totals, in sorted order j: its positions, the caller's index and where its token log-probs go
struct RnnLmHyp {
    int npos = 0, orig = 0;
    long long out_off = 0;
};
// one wave per hypothesis j: total = the float32 sum of lp[base[t] + j] over t < npos in position order -> totals[orig]; the same
// values -> token_log_probs[out_off + t] when token_log_probs is not null
void rnn_lm_totals(const Ctx& ctx, const float* lp, const RnnLmHyp* hyps, const long long* base, int Hn, float* token_log_probs, float* totals);

// ---- decoder / joiner / greedy ----------------------------------------------------
struct DecJoinW {
    const float* emb;      // [V, DD]
    const float* conv;     // [DD, cpg, ctx] (cpg <= 4) or k-major [cpg*ctx][DD] (cpg > 4)
    int cpg;               // decoder conv input channels per group
    // groups = 1 only: per-token conv contributions P[tap][v][co] = sum_ci conv[co][ci][tap] * emb[v][ci]  ([2][V][DD]);
    // the conv of a context is then relu(P[0][y0] + P[1][y1]) -- no GEMV inside the search loops
    const float* ptab = nullptr;
    const float* dproj_kn; // [DD, J]
    const float* dproj_b;  // [J]
    const float* out_kn;   // [J, Vp]
    const float* out_b;    // [V]
    // small vocabularies only: decoder(y0, y1) of EVERY context, row (y0 + 1) V + y1 of [(V + 1) V][J], y0 = -1 .. V-1 (decoder_table);
    // the search kernels then read a row where they would run the decoder
    const float* dec_table = nullptr;
    // large vocabularies only (model.cpp add_repacks): output_linear as f16 in MFMA fragment order + the per-column bound on
    // |f16 product - f32 logit| -- the greedy search's screening pass (greedy.hip screen_round); null = every round sweeps in f32
    const void* out_h16 = nullptr;
    const float* out_eps = nullptr;
    const float* out_vj = nullptr;   // output_linear in its torch layout [V][J]: a candidate column's weights in one 2 KB piece (the re-check)
    int V, Vp, DD, J, ctx;
};
void decoder(const Ctx& ctx, const DecJoinW& w, const long long* y, int N, float* dec_out);
// out[2][J] = the search kernel's own decoder routine on [-1, blank] and [blank, blank] (bit-identical to what k_greedy computes itself)
void decoder_start_contexts(const Ctx& ctx, const DecJoinW& w, float* out);
// table[(V + 1) V][J]: the search kernels' decoder routine on every context (bit-identical to what they compute themselves)
void decoder_table(const Ctx& ctx, const DecJoinW& w, float* table);
// out[N][J] = that routine on the contexts y[N][2], computed (the table is not consulted): what the table's rows are checked against
void decoder_rows_wide(const Ctx& ctx, const DecJoinW& w, const long long* y, int N, float* out);
void tanh_add(const Ctx& ctx, const float* enc, const float* dec, int dec_stride, float* y, int N, int J);
// row argmax with the reference tie-break (later index wins) -> emit flag (token not in {0,2} [,1])
void argmax_rows(const Ctx& ctx, const float* logits, int ld, int N, int V, int* tok);
// ---- CTC (zipformer2ctc models) ------------------------------------------------------------------
void log_softmax_rows(const Ctx& ctx, float* x, int M, int V);  // in place
// Array.IndexOf(row, row.Max()): the FIRST index of the maximum (OfflineRecognizer.cs:388)
void argmax_first_rows(const Ctx& ctx, const float* logits, int ld, int N, int V, int* tok);
// per stream: drop blanks and repeats (prev_id = -1), timestamp = t + frame_off[b]; trail[b] = blank frames at the end,
// any[b] = 1 if some frame was non-blank (OfflineRecognizer.cs:383-408)
void ctc_collapse(const Ctx& ctx, const int* tok, int B, int Tp, const int* frame_off, long long* tokens, int* timestamps,
                  int* n_tokens, int max_tokens, int* trail, int* any, int* overflow);
// t0 = first frame at which any stream emits under the initial context
void first_emit_frame(const Ctx& ctx, const int* tok, int B, int Tp, int skip1, int* t0);
struct GreedyArgs {
    const float* enc;   // [B, Tp, J]
    int B, Tp;
    const int* t0;      // device scalar (batch quirk) or nullptr (single path)
    int skip1;          // online filter also skips id 1
    int max_sym;        // 1000 for the single path, else INT_MAX
    long long* tokens;  // [B, max_tokens]
    int* timestamps;    // [B, max_tokens]
    int* n_tokens;      // [B]
    int max_tokens;
    int* overflow;      // device flag
    // online loop: per-stream starting context (stream.Hyp, OnlineRecognizer.cs:109,122-126); null = offline
    const long long* init_ctx = nullptr;  // [B][2]
    // vocabulary-parallel form (set by greedy_loop): `parts` workgroups per stream, each sweeping a slab of the joiner
    // matrix; per round they exchange their per-frame (max, argmax) through tagged 8-byte granules
    int parts = 1;
    unsigned long long* gran = nullptr;  // [B][2 (round parity)][parts][GF][2], zeroed per call
    unsigned long long* gran2 = nullptr;  // [B][2 (emission parity)][J]: the parts' slices of a decoder update, zeroed per call
    // decoder outputs of the two start contexts [-1, blank] and [blank, blank] ([2][J], from decoder_start_contexts): constants of
    // the model, so every workgroup of every batch loads them instead of running the decoder twice (null: computed in the kernel)
    const float* dec_init = nullptr;
    // tuning only (K2HIP_GREEDY_STAMPS): workgroup 0 accumulates s_memrealtime (100 MHz) differences per phase of a round here --
    // [0] rounds, [1] activations, [2] screen tiles, [3] candidate scan, [4] re-check, [5] sweep passes, [6] publish + exchange,
    // [7] decision + decoder update
    unsigned long long* stamps = nullptr;
    // K2HIP_SCREEN_COUNT: [2] device counters, or nullptr (no atomics in the kernel).  Thread 0 of every part adds one per round of the
    // large-vocabulary instantiation: [0] the f16 screen decided the round, [1] the round ran the f32 passes (the screen gave up, or
    // the part's slab does not fit it)
    unsigned long long* screen_counts = nullptr;
};
void greedy_loop(const Ctx& ctx, const DecJoinW& w, const GreedyArgs& a);
bool greedy_loop_screens(const DecJoinW& w, int B, bool streaming, bool one_part);  // would its rounds use the f16 screen (large vocabulary, slab fits)?
// The vocabulary-parallel search waits on its sibling workgroups (bounded spins; a timeout raises *overflow = 2).  All B x parts
// workgroups must be resident together for that, which a GPU shared with other processes or models does not promise.  The engine
// therefore keeps the launch (inputs are read-only, outputs are rewritten from scratch) and, on a timeout, runs it again with ONE
// workgroup per stream -- no inter-workgroup wait, same tokens -- instead of failing the call.
// arguments of the one-kernel modified beam search (beam.hip k_beam_loop); here because a repeatable launch is kept in GreedyLaunch
// One stream's hotword graph as the search reads it: the dense tables on the device (BeamArgs::hw_*).  All null: this stream is
// unbiased -- no bonus, its hypotheses stay in state 0.
struct BeamHwStream {
    const int* next = nullptr;
    const float* bonus = nullptr;
    const float* pending = nullptr;
};
// The n-gram LM of the search (shallow fusion) as the kernels read it: the sparse form of ngram_lm.h on the device, every weight already
// multiplied by the scale (the device only adds).  states == null: no LM.  states [S] = (arc begin, arc end, back-off state, back-off
// weight bits) -- one 16-byte load per level of a walk; the arcs of a state sorted by token; uni_* [V]: state 0 as a dense row with
// the <unk> rule resolved, so every walk ends in one direct load.
struct BeamLm {
    const int4* states = nullptr;
    const int* arc_tok = nullptr;
    const float* arc_lp = nullptr;
    const int* arc_next = nullptr;
    const float* uni_lp = nullptr;
    const int* uni_next = nullptr;
    int start = 0;   // the start hypothesis' state
};
// N-best outputs of the offline search (device; tokens == null: off): up to `nbest` final hypotheses per stream in the order of the
// final pick, (finalized log-prob) / (length + 2) descending with ties in insertion order -- entry 0 is the single result
struct BeamNbest {
    int nbest = 0;
    long long* tokens = nullptr;        // [B][nbest][max_tokens]
    int* timestamps = nullptr;          // [B][nbest][max_tokens]
    float* token_log_probs = nullptr;   // [B][nbest][max_tokens]
    int* n_tokens = nullptr;            // [B][nbest]
    float* scores = nullptr;            // [B][nbest] finalized log-probs (not normalised)
    int* n_hyps = nullptr;              // [B] entries written: min(survivors, nbest)
};
struct BeamLoopArgs {
    const float* enc;   // [B, Tp, J]
    int Tp, K, cap;
    long long* tokens;
    int* timestamps;
    int* n_tokens;
    float* scores;
    int max_tokens;
    int* overflow;
    // long utterances: the hypotheses' token / timestamp arrays do not fit in LDS beside the logits and live in device memory,
    // [B][2][K][cap] each (a workgroup reads back only what it wrote itself: one CU, one L1); null = in LDS
    int* ys_g;
    int* ts_g;
    // two column slabs per stream (beam <= 4, 256 < V <= 512): workgroup 2 b + p sweeps chunk p and the two exchange their 4 x 256
    // logits per frame as tagged granules xg[b][frame parity][slab][4][256]; null = one workgroup per stream
    unsigned long long* xg;
    int* trace = nullptr;   // debug tap [B][Tp][2 K + 1] (beam_step_body) or null
    // streaming resume (BeamResume below): per-stream in / out blocks, or null for the offline search
    const int* rin = nullptr;
    int* rout = nullptr;
    // hotword biasing (BeamArgs below) or null pointers: one graph for every stream (hw_*), or one per stream (hw_streams) with
    // the saved hypotheses' states in / the survivors' states out (resume only)
    const int* hw_next = nullptr;
    const float* hw_bonus = nullptr;
    const float* hw_pending = nullptr;
    const BeamHwStream* hw_streams = nullptr;
    const int* st_in = nullptr;
    int* st_out = nullptr;
    BeamLm lm;   // n-gram LM or null tables; resume: the saved hypotheses' LM states in / the survivors' out [B][K]
    const int* lst_in = nullptr;
    int* lst_out = nullptr;
    // token log-probs (false: not kept): yp beside ys / ts -- in LDS, or yp_g [B][2][K][cap] where ys_g / ts_g are used; nb: the
    // offline N-best outputs; yp_out: the resumed search's side block [B][K][Tp], the token log-probs of each survivor's suffix
    bool want_yp = false;
    float* yp_g = nullptr;
    BeamNbest nb;
    float* yp_out = nullptr;
};
struct GreedyLaunch {
    bool valid = false;  // a launch with inter-workgroup waits (parts > 1 / two beam slabs) that can be repeated without them
    DecJoinW w;
    GreedyArgs a;        // (beam: only B and overflow are meaningful)
    bool beam = false;   // the launch was k_beam_loop with two slabs per stream: ba, beam_lds
    BeamLoopArgs ba;
    size_t beam_lds = 0;
};
void beam_relaunch_one_slab(hipStream_t stream, const GreedyLaunch& rec);
void greedy_relaunch_one_part(hipStream_t stream, const GreedyLaunch& rec);
// The same search as batched ROUNDS instead of one persistent workgroup pair per stream: every round evaluates the next S frames
// of every stream under the stream's current context with ONE joiner GEMM over all B x S rows, then a per-stream step accepts
// frames up to and including the first emission, updates the context, runs the decoder if it changed and forms the next
// window's tanh(enc + dec) rows.  Exactly the frame-by-frame loop (frames behind an emission are re-evaluated in the next round);
// max(Tp) rounds are enqueued up front, rounds after the last stream has finished return at their first instruction.
// out_w: joiner.output_linear.weight [V, J] (torch layout, for the GEMM).  Batch / online semantics only (no max_sym cap).
void greedy_rounds(const Ctx& ctx, const DecJoinW& w, const float* out_w, const GreedyArgs& a);

// ---- modified beam search (beam.hip) ------------------------------------------------------------
constexpr int kMaxBeam = 8;
// A search that resumes from saved hypotheses (streaming: one chunk of Tp frames per call).  Hypothesis j of the saved set is
// H_j (its whole token sequence, which only the host keeps); inside the chunk a hypothesis is (saved index, suffix of <= Tp tokens).
// Two candidates from different saved hypotheses spell the same sequence only if one saved sequence is the other plus a short
// suffix x: rel[a][b] = |x| when H_a = H_b + x with 0 < |x| <= Tp (x = relx[a][b]), else -1 (0 on the diagonal).
// Per stream, `in` (ints):  [nhyp | lp[K] (float bits) | ctx[K][2] | len[K] (|H_j|) | rel[K][K] | relx[K][K][Tp]]
//             `out` (ints): [nhyp | best | org[K] | n[K] | lp[K] (float bits) | ctx[K][2] | ys[K][Tp] | ts[K][Tp] (chunk-relative)]
struct BeamResumeLayout {
    int K, Tp;
    __host__ __device__ int in_ints() const { return 1 + 4 * K + K * K + K * K * Tp; }
    __host__ __device__ int in_lp() const { return 1; }
    __host__ __device__ int in_ctx() const { return 1 + K; }
    __host__ __device__ int in_len() const { return 1 + 3 * K; }
    __host__ __device__ int in_rel() const { return 1 + 4 * K; }
    __host__ __device__ int in_relx() const { return 1 + 4 * K + K * K; }
    __host__ __device__ int out_ints() const { return 2 + 5 * K + 2 * K * Tp; }
    __host__ __device__ int out_org() const { return 2; }
    __host__ __device__ int out_n() const { return 2 + K; }
    __host__ __device__ int out_lp() const { return 2 + 2 * K; }
    __host__ __device__ int out_ctx() const { return 2 + 3 * K; }
    __host__ __device__ int out_ys() const { return 2 + 5 * K; }
    __host__ __device__ int out_ts() const { return 2 + 5 * K + K * Tp; }
};
struct BeamState {       // device arrays; hypotheses double-buffered by frame parity
    int K, cap;
    int* org = nullptr;  // [2][B][K] saved-hypothesis index of each hypothesis (resume only)
    const int* rin = nullptr;   // resume in blocks [B][in_ints] or null
    int Tp = 0;
    int* ys;             // [2][B][K][cap] tokens without the ctx-blank prefix
    int* ts;             // [2][B][K][cap]
    float* yp = nullptr; // [2][B][K][cap] token log-probs, parallel to ts (null: not kept)
    float* yp_out = nullptr;   // resume: side block [B][K][Tp] (null: not asked for)
    int* n;              // [2][B][K]
    float *lp, *lp_next; // [B][K] hypothesis log-probs (-inf = empty slot)
    long long *ctx, *ctx_next;  // [B][K][2] decoder inputs
    int *nhyp, *nhyp_next;      // [B]
    // hotword biasing: the hypotheses' graph states [2][B][K] and the tables (one graph, or hw_streams [B]: one per stream), or null;
    // resume: the saved hypotheses' states st_in [B][K], the survivors' st_out [B][K]
    int* st = nullptr;
    const int* hw_next = nullptr;
    const float* hw_bonus = nullptr;
    const float* hw_pending = nullptr;
    const BeamHwStream* hw_streams = nullptr;
    const int* st_in = nullptr;
    int* st_out = nullptr;
    // n-gram LM: the hypotheses' LM states [2][B][K] beside st, and the tables (null: none)
    int* lst = nullptr;
    BeamLm lm;
    const int* lst_in = nullptr;
    int* lst_out = nullptr;
    // neural LM shallow fusion (null: none), slot-indexed over M = B K: the hypotheses' next-token log-probs nq [2][M][V] by frame
    // parity, what the step writes for the LM launches behind it -- npar [M] the slot (of the other parity) each new slot continues,
    // ntok [M] the token it appended or -1 -- and nflag [Tp]: frame t's "some slot appended" flag
    const float* nq = nullptr;
    int* npar = nullptr;
    int* ntok = nullptr;
    int* nflag = nullptr;
    float nscale = 0.f;
    // LODR (the neural instantiation only): the hypotheses' states of the second automaton [2][B][K] beside lst, its tables (every
    // weight times the scale <= 0; null: none) and the resumed search's side blocks.  (Behind everything else: the members the other
    // instantiations read keep their place in the kernels' argument block.)
    int* dst = nullptr;
    BeamLm lodr;
    const int* dst_in = nullptr;
    int* dst_out = nullptr;
};
struct BeamArgs {
    const float* enc;    // [B, Tp, J]
    const float* out_w;  // joiner.output_linear.weight [V, J] (torch layout, for the GEMM)
    const float* dproj_w;  // joiner.decoder_proj.weight [J, DD] (torch layout)
    int B, Tp, beam;
    long long* tokens;   // [B, max_tokens] best hypothesis
    int* timestamps;
    int* n_tokens;
    float* scores;       // [B] log_prob of the best hypothesis (may be null)
    int max_tokens;
    int* overflow;
    int* trace = nullptr;  // debug tap [B][Tp][2 beam + 1] or null (k2hip_debug.h: k2hip_debug_beam_trace)
    // streaming resume (BeamResumeLayout): start from the saved hypotheses in rin [B][in_ints] instead of [blank, blank] and write
    // every surviving hypothesis to rout [B][out_ints] instead of the best one to tokens / timestamps / n_tokens / scores
    const int* rin = nullptr;
    int* rout = nullptr;
    // Hotword biasing (hotwords.h; semantics in include/k2hip.h): the dense tables of the graph on the device --
    // hw_next [S][V] the state after appending a token (the root after a committed match), hw_bonus [S][V] what the step adds to the
    // hypothesis' log-prob, hw_pending [S] what the final pick takes back from an unfinished match.  Every hypothesis carries its
    // state; the bonus of a selected candidate is added after the frame's selection and before the merges.  Null: the unbiased search
    // (its own template instantiations of the kernels: today's arithmetic, nothing added).
    const int* hw_next = nullptr;
    const float* hw_bonus = nullptr;
    const float* hw_pending = nullptr;
    // The streaming form (with rin / rout): one graph PER STREAM, hw_streams [B] on the device (a stream without a graph: null
    // tables), instead of hw_*; st_in [B][K] the graph states of the saved hypotheses, st_out [B][K] those of the survivors (0 for
    // empty slots).  `best` of the out block is then picked on (lp - pending(state)) / length; the log-probs written keep the
    // pending bonus (the match may complete in the next chunk).
    const BeamHwStream* hw_streams = nullptr;
    const int* st_in = nullptr;
    int* st_out = nullptr;
    // N-gram LM shallow fusion (ngram_lm.h; semantics in include/k2hip.h): every hypothesis carries an LM state beside its hotword
    // state; a selected candidate that appends a real token gets (sum + hotword bonus) + Step(state, token) before the merges, nothing
    // is taken back at the end.  Runs in the biased instantiations (a null check there, as for hw_bonus).  The resumed search takes
    // the saved hypotheses' LM states in lst_in [B][K] and writes the survivors' to lst_out [B][K], side blocks as st_in / st_out are.
    BeamLm lm;
    const int* lst_in = nullptr;
    int* lst_out = nullptr;
    // Neural LM shallow fusion (rnn_lm_fuse.hip; semantics in include/k2hip.h): every hypothesis carries the LSTM state of its token
    // sequence and the LM's next-token log-probs; a selected candidate that appends a real token v gets
    // ((sum + hotword bonus) + n-gram term) + fl32(scale q_parent[v]) before the merges.  Offline only, always in the per-frame launch
    // form; nlm.dev.emb == null: off.  Resumed (rin set): nlm_io [B] names the streams' state blocks (NlmStreamIO), the LM launches
    // run behind EVERY frame and the movers of rnn_lm_fuse.hip frame the call.
    BeamNlm nlm;
    const NlmStreamIO* nlm_io = nullptr;
    // LODR (semantics in include/k2hip.h): a second automaton, the low-order LM with every weight multiplied by its scale <= 0, walked
    // beside the n-gram LM's with a state of its own per hypothesis; its term is added last, ((.. + n-gram term) + neural term) +
    // Step_lodr(state, token).  Only beside the neural LM (nlm on); lodr.states == null: none.  Resumed: the saved hypotheses' states
    // in dst_in [B][K], the survivors' out dst_out [B][K], side blocks as lst_in / lst_out are.
    BeamLm lodr;
    const int* dst_in = nullptr;
    int* dst_out = nullptr;
    // Token log-probs and N-best (semantics in include/k2hip.h).  Both null: nothing is kept beyond the best hypothesis.  nb: the
    // offline search also writes its final hypotheses in pick order; yp_out [B][K][Tp] (resume): the token log-probs of each
    // survivor's suffix, a side block beside rout as st_out is.
    BeamNbest nb;
    float* yp_out = nullptr;
    // Set with either of them.  The sizing pass (Ctx::dry) hands out null pointers, so nb.tokens / yp_out cannot tell it that the
    // search will keep token log-probs: without this flag it sized the arena without the [2][B][K][cap] array beside ys / ts.
    bool keep_yp = false;
};
// launches of the search since the process started, by instantiation: [0] HW = false, [1] HW = true (k2hip_debug.h)
void beam_launch_counts(long long* plain, long long* hw);
void beam_search(const Ctx& ctx, const DecJoinW& w, const BeamArgs& a);

// ---- forced alignment and full-sum scoring on the RNN-T lattice (align.hip; semantics in include/k2hip.h and lattice_ref.h) ----
// One stream of an align call: T frames (the first T of its Tp encoder rows), U target tokens, its U + 1 contexts at rows ctx_off ..
// of the call's decoder outputs, its targets at ids[id_off ..], its two planes [T][U + 1] at plane_off floats into stay / emit, and
// its back-pointer bits [T][ceil((U + 1) / 64)] 64-bit words at bp_off words into bp.
struct AlignStream {
    long long plane_off, bp_off;
    int ctx_off, id_off, U, T;
};
struct AlignArgs {
    const float* enc = nullptr;          // [B, Tp, J]
    int B = 0, Tp = 0;
    int max_T = 0, max_U = 0;            // over the call's streams (the launch grid)
    const AlignStream* streams = nullptr;   // [B] (device)
    const int* ids = nullptr;            // the targets back to back (device); lattice_dp: may be null
    const float* dec = nullptr;          // [sum(U_b + 1)][J]: decoder() of every position's context
    float *stay = nullptr, *emit = nullptr;
    unsigned long long* bp = nullptr;
    // lattice_dp's results: tokens / timestamps / token_log_probs [B][max_tokens] (tokens: the targets back, may be null), n_tokens [B]
    // (= U, may be null), scores [B][2] = (total, best)
    long long* tokens = nullptr;
    int* timestamps = nullptr;
    float* token_log_probs = nullptr;
    int* n_tokens = nullptr;
    float* scores = nullptr;
    int max_tokens = 0;
};
// stay(t,u) = logaddexp(lp(t,u,blank), lp(t,u,unk)) and emit(t,u) = lp(t,u,y_{u+1}) of every cell of the reachable band, with
// lp = log_softmax(output_linear(tanh(enc[t] + dec[u]))) swept on the f32 matrix pipe -- no logits are stored.  emit(t,U) = -inf.
void lattice_logprobs(const Ctx& ctx, const DecJoinW& w, const AlignArgs& a);
// forward (logaddexp) and Viterbi (max, emit wins ties) recursions over the two planes, one workgroup per stream, then the backtrace
constexpr int kAlignMaxU = 4095;   // U + 1 positions of both recursions' two rows live in LDS
void lattice_dp(const Ctx& ctx, const AlignArgs& a);

// ---- keyword spotting: trie Viterbi on the transducer lattice (kws.hip; semantics in include/k2hip.h and kws_ref.h) ----
// A keyword graph resident on the device (keywords.h): the decoder row of every state's context and the trie's tables.
struct KwsGraphDev {
    const float* dec = nullptr;          // [S][J]: decoder() of ctx(s)
    const int* parent = nullptr;         // [S]
    const int* depth = nullptr;          // [S]
    const int* kw = nullptr;             // [S], -1 = no keyword ends there
    const float* bar = nullptr;          // [S]
    const int* child_off = nullptr;      // [S + 1]
    const int* child_tok = nullptr;      // [S - 1], sorted by token inside every state's range
    const int* child_state = nullptr;    // [S - 1]
    int S = 0;
};
// One stream of a chunk call: T frames (the first T of its Tp encoder rows; 0 = the stream is carried through unchanged), its two planes
// [T][S] at plane_off floats into stay / emit, its carried block [S] at state_off into a_in / start_in / a_out / start_out.
struct KwsStream {
    KwsGraphDev g;
    long long plane_off;
    int state_off, T;
};
struct KwsArgs {
    const float* enc = nullptr;          // [B, Tp, J]
    int B = 0, Tp = 0;
    int max_T = 0, max_S = 0;            // over the call's streams (the launch grid, the DP's LDS rows)
    const KwsStream* streams = nullptr;  // [B] (device)
    float *stay = nullptr, *emit = nullptr;
    const float* a_in = nullptr;
    const int* start_in = nullptr;
    float* a_out = nullptr;
    int* start_out = nullptr;
    // trie_dp's events, row b of [B][max_events] each (max_events >= max_T: at most one per frame), n_events [B]
    long long* ev_keyword = nullptr;
    int *ev_end = nullptr, *ev_start = nullptr;
    float* ev_sum = nullptr;
    int* n_events = nullptr;
    int max_events = 0;
};
constexpr int kKwsMaxStates = 1024;   // = K2HIP_KEYWORDS_MAX_STATES: four states per lane of trie_dp's workgroup
// stay(t,s) = logaddexp(lp(t,s,blank), lp(t,s,unk)) of every state and emit(t,c) = lp(t,parent(c),tok(c)) of every non-root state (column
// 0 of emit: -inf), lp = log_softmax(output_linear(tanh(enc[t] + dec[s]))) swept on the f32 matrix pipe -- no logits are stored
void trie_logprobs(const Ctx& ctx, const DecJoinW& w, const KwsArgs& a);
// token passing over the two planes, one workgroup per stream: the carried block in, events and the new carried block out
void trie_dp(const Ctx& ctx, const KwsArgs& a);

// ---- keyword spotting for CTC models: trie Viterbi on the CTC trellis (ctc_kws.hip; semantics in include/k2hip.h and ctc_kws_ref.h) ----
// One stream of a chunk call: its graph's tables [parent | tok | depth | kw | bar | rc], each [S] words (rc(s) = the root's child whose
// token is tok(s), or -1), at table_off words into `tables`; the first T frames of row `row` of log_probs (0 = the stream is carried
// through unchanged); its carried block -- values [2][S] and starts [2][S], plane 0 = n, plane 1 = b -- at 2 * state_off into v_in /
// st_in / v_out / st_out.
struct CtcKwsStream {
    int table_off, S, row, state_off, T;
};
struct CtcKwsArgs {
    const float* log_probs = nullptr;    // [R, Tp, V]
    int B = 0, Tp = 0, V = 0;
    int max_T = 0, max_S = 0;            // over the call's streams
    const CtcKwsStream* streams = nullptr;   // [B] (device)
    const int* tables = nullptr;             // the call's distinct graphs, back to back (device)
    const float* v_in = nullptr;
    const int* st_in = nullptr;
    float* v_out = nullptr;
    int* st_out = nullptr;
    // the events, row b of [B][max_events] each (max_events >= max_T: at most one per frame), n_events [B]
    long long* ev_keyword = nullptr;
    int *ev_end = nullptr, *ev_start = nullptr;
    float* ev_sum = nullptr;
    int* n_events = nullptr;
    int max_events = 0;
};
// token passing over the log-probs, one workgroup per stream: the carried block in, events and the new carried block out
void ctc_trie_dp(const Ctx& ctx, const CtcKwsArgs& a);

// ---- CTC forced alignment and full-sum scoring (ctc_align.hip; semantics in include/k2hip.h and ctc_lattice_ref.h) ----
// One target of a CTC align call: U tokens at ids[id_off ..], scored against row `row` of log_probs over its first T frames; its compact
// plane [T][U + 1] (column 0: lp(t, blank), column k: lp(t, y_k)) at plane_off floats into `plane`, and its back-pointers
// [T][ceil(S / 64)][2] 64-bit words (S = 2U + 1; the low and the high bit of every state's two-bit pointer) at bp_off words into bp.
struct CtcAlignTarget {
    long long plane_off, bp_off;
    int row, id_off, U, T;
};
struct CtcAlignArgs {
    const float* log_probs = nullptr;    // [R, Tp, V], log-softmaxed
    int Tp = 0, V = 0, H = 0;
    int max_T = 0, max_U = 0;            // over the call's targets (the launch grid, the LDS rows)
    const CtcAlignTarget* targets = nullptr;   // [H] (device)
    const int* ids = nullptr;            // the targets back to back (device)
    float* plane = nullptr;
    unsigned long long* bp = nullptr;
    // results: tokens / timestamps / end_frames / token_log_probs [H][max_tokens] (tokens: the targets back, may be null), n_tokens [H]
    // (= U, may be null), scores [H][2] = (total, best)
    long long* tokens = nullptr;
    int *timestamps = nullptr, *end_frames = nullptr;
    float* token_log_probs = nullptr;
    int* n_tokens = nullptr;
    float* scores = nullptr;
    int max_tokens = 0;
};
constexpr int kCtcAlignMaxTokens = 4095;   // = kCtcAlignMaxU of ctc_lattice_ref.h: four rows of 2U + 1 floats live in LDS (131 KB)
// gather pass (the U + 1 columns every target needs, out of [Tp][V] into its compact plane), then one workgroup per target: forward
// (logaddexp) and Viterbi (max, the lowest state index wins ties) over the reachable band, two back-pointer bits per cell, backtrace
void ctc_lattice(const Ctx& ctx, const CtcAlignArgs& a);

// ---- CTC prefix beam search with N-best (ctc_prefix.hip; semantics in include/k2hip.h and ctc_prefix_ref.h) ----
struct CtcPrefixArgs {
    const float* log_probs = nullptr;   // [R, Tp, V], log-softmaxed
    int R = 0, Tp = 0, V = 0;           // V is the call's (the debug op runs other vocabularies than the model's)
    const int* n_frames = nullptr;      // [R] (device) or null = Tp for every row
    int beam = 0;                       // 1 .. kMaxBeam
    int4* nodes = nullptr;              // history pool [R][Tp * beam]: (parent, token, frame, token log-prob bits); parent -1 = the empty prefix
    // the best hypothesis of every row (the search-output block) and its score
    long long* tokens = nullptr;        // [R][max_tokens]
    int* timestamps = nullptr;          // [R][max_tokens]
    int* n_tokens = nullptr;            // [R]
    float* scores = nullptr;            // [R]
    int max_tokens = 0;
    int* overflow = nullptr;            // set to 1 when a written entry is longer than max_tokens (that entry is not written)
    BeamNbest nb;                       // tokens == null: off; else the first min(nb.nbest, live) slots in rank order
};
// One workgroup of 256 per row, frames sequential, no workgroup waits for another; every store is an ordinary vector store
void ctc_prefix_search(const Ctx& ctx, const CtcPrefixArgs& a);
// The same search with hotword and n-gram LM biasing (include/k2hip.h "Hotword and n-gram LM biasing of the CTC prefix beam search"): the
// dense hotword tables [S][V] / [S] and the scaled sparse LM as the modified beam search reads them.  All of hw null / lm.states null:
// that half adds nothing.  The caller has checked that every state the tables name is inside them (ctc_prefix_bias_ref.h).
struct CtcPrefixBiasArgs : CtcPrefixArgs {
    BeamHwStream hw;
    BeamLm lm;
};
void ctc_prefix_search_biased(const Ctx& ctx, const CtcPrefixBiasArgs& a);
// The search resumed from the live prefixes of the chunks before (streaming: one chunk of <= Tc frames per call).  Carried slot a is
// the prefix S_a, whose tokens only the host keeps (ctc_prefix_hist.h); inside the chunk a prefix is (carried slot, suffix of <= Tc
// tokens).  rel[a][b] = |x| when S_a = S_b + x with 0 < |x| <= Tc (x = relx[a][b]), else -1 (0 on the diagonal), as BeamResumeLayout.
// The hashes are the kernel's own rolling hashes of the prefix and of the prefix without its last token, passed back as they came out.
// Per stream, `in` (ints):  [n | pb[K] | pnb[K] (float bits) | e[K] (last token, -1: empty) | len[K] | hash[K][2] | phash[K][2] (lo, hi) |
//                            rel[K][K] | relx[K][K][Tc]]
//             `out` (ints): [n | org[K] | napp[K] | pb[K] | pnb[K] (float bits) | hash[K][2] | phash[K][2] | tot[K] (float bits: the score) |
//                            ys[K][Tc] | ts[K][Tc] (chunk-relative) | yp[K][Tc] (float bits)], the survivors in rank order
// (CtcPrefixResumeLayout{K, Tc}: ctc_prefix_layout.h, shared with the host history ctc_prefix_hist.h)
struct CtcPrefixResumeArgs {
    const float* log_probs = nullptr;   // [B, Tc, V], log-softmaxed
    int B = 0, Tc = 0, V = 0;
    const int* n_frames = nullptr;      // [B] (device), each in [1, Tc], or null = Tc for every stream
    int beam = 0;                       // 1 .. kMaxBeam: K of the layout
    int4* nodes = nullptr;              // in-chunk history pool [B][Tc * beam]; a parent < 0 is the carried slot -1 - parent
    const int* in = nullptr;            // [B][in_ints]
    int* out = nullptr;                 // [B][out_ints]
    int* status = nullptr;              // set to 1 when an in block contradicts itself (a bounded walk ran into its bound)
};
void ctc_prefix_resume(const Ctx& ctx, const CtcPrefixResumeArgs& a);
// The resumed search with per-stream hotword graphs and the call's n-gram LM (include/k2hip.h "Biasing of the streaming CTC prefix beam
// search").  The in / out blocks above are unchanged (tot there stays acoustic); the slots' (ctx, hs, ls) come in and the survivors'
// (ctx, hs, ls, fin, ord) go out through side blocks of their own (CtcPrefixResumeBiasLayout{K}).  hw_streams [B] on the device: a row's
// dense tables, all null = no graph for that row; a row runs the LM only if its side in block sets flag bit 0.  A row with neither is
// bit for bit the plain resumed search.  The caller has checked every table and every carried hs / ls against its table.
struct CtcPrefixResumeBiasArgs : CtcPrefixResumeArgs {
    const BeamHwStream* hw_streams = nullptr;   // [B] (device)
    BeamLm lm;
    const int* side_in = nullptr;               // [B][in_ints]
    int* side_out = nullptr;                    // [B][out_ints]
};
void ctc_prefix_resume_biased(const Ctx& ctx, const CtcPrefixResumeBiasArgs& a);

// ---- streaming (online.hip): device-resident per-stream caches indexed by slot ------------------
// ConvNeXt.streaming_forward's data movement in one launch: cat[b] = [cached_left_pad ; x], the cache advanced to x's frames Tc-3 .. Tc-1,
// byp[b] = x[b, :Tc] (the bypass operand)
void convnext_cat(const Ctx& ctx, const float* a3, float* pool, long long slot_stride, long long embed_off, const int* slots, float* cat,
                  float* byp, int B, int T3, int Tc, int F, int C);
// tanh_gated: the new rows are formed as x[width + c] * tanh(x[c]) from rows of >= 2*width floats (NonlinAttention's gated input)
void cat_shift(const Ctx& ctx, float* pool, long long slot_stride, long long off, const int* slots, const float* newrows,
               int ldn, float* cat, int B, int L, int Tc, int width, bool tanh_gated = false);
// ring form: the keys of the left context are read from the ring, the chunk's own key rows (columns [32 H, 64 H) of qkp) are
// written into it first; aw columns are in RING order (column p = the key stored in ring row p), which is also the order the
// value rings are read in -- a weighted sum does not care.
// the same with `keep_back` newest rows kept OUT of the cache (streaming Conformer with right_context: states = key[-(L + R) : -R]):
// cat = [cache ; new rows] first, then cache <- cat[Tc - keep_back .. Tc - keep_back + L) (two launches: the cache is read before it is written)
void cat_keep(const Ctx& ctx, float* pool, long long slot_stride, long long off, const int* slots, const float* newrows, int ldn, float* cat,
              int B, int L, int Tc, int width, int keep_back);
void attn_stream_ring(const Ctx& ctx, const float* qkp, int ld, const RingRef& keys, const float* pp, const long long* plen,
                      float* aw, int B, int Tc, int L, int KLp, int H, int ds, int left50);
void attn_stream(const Ctx& ctx, const float* qkp, int ld, const float* kcat, const float* pp, const long long* plen,
                 float* aw, int B, int Tc, int L, int KLp, int H, int ds, int left50);
void glu_causal_conv(const Ctx& ctx, const float* x2, float* pool, long long slot_stride, long long off, const int* slots,
                     const float* wc, const float* bc, const float* ww, const float* bw, const float* sc, float* y, int B,
                     int Tc, int D, int K);
// Device mirror of the streams' feature FIFOs (OnlineStream's Speech): fifo [slots][cap][feat] rings.
//   fifo_append: frames [g][0 .. nf) of `src` go to ring rows (pos[g] + i) % cap of slot slots[g] (pos[g] < 0: skipped)
//   fifo_gather: x[b][t] = ring row (head[b] + t) % cap of slot slots[b], t < T  -- the chunk input of a step, no host round trip
void fifo_append(const Ctx& ctx, float* fifo, int cap, int feat, const float* src, const int* slots, const int* pos, int G, int nf);
// (the gathered frames pass the online PadSequence's floor of genuine zeros on the way: PadHelper.cs:9-13,58)
void fifo_gather(const Ctx& ctx, const float* fifo, int cap, int feat, const int* slots, const int* head, float* x, int B, int T);
void zero_floats(const Ctx& ctx, float* p, long long n);
// ---- streaming Zipformer v1 (zipformer1.hip; OnlineProjOfZipformer) ------------------------------
// running mean over every frame seen so far: out [B*Tc, D]; cached_avg (avg_off, [D]) and cached_len (len_off, 1 float) per slot
void z1_pool(const Ctx& ctx, const float* x, float* pool, long long slot_stride, long long avg_off, long long len_off, const int* slots,
             float* out, int B, int Tc, int D);
// qkvp rows (ld): q [A] | k [A] | v [A/2] | p [H*4]; kcat [B, L+Tc, A]; pp [2Tc-1+L, H*4]; aw out [H][B][Tc][KLp]
void z1_attn(const Ctx& ctx, const float* qkvp, int ld, const float* kcat, const float* pp, float* aw, int B, int Tc, int L, int KLp,
             int H, int A);
// y = DoubleSwish(dwconv_K([cache ; glu(x2)]) + bias); cache [D][K-1] per slot at `off`, updated
void z1_glu_conv(const Ctx& ctx, const float* x2, float* pool, long long slot_stride, long long off, const int* slots, const float* w,
                 const float* bias, float* y, int B, int Tc, int D, int K);
// y = orig + (BasicNorm(x) - orig) * bypass_scale (scalar)
void z1_norm_bypass(const Ctx& ctx, const float* x, const float* orig, const float* log_eps, const float* bscale, float* y, int M, int D);
// AttentionDownsample, first Din channels: x [B,T,Din] -> y [B,ceil(T/ds),ldy]
void z1_attn_downsample(const Ctx& ctx, const float* x, const float* query, float* y, int B, int T, int Din, int ldy, int ds);
// offline graph: mean over the utterance's frames [B,D]; x[b,t,:] += v[b,:]; the ds frames of a downsampling group side by side
void z1_mean(const Ctx& ctx, const float* x, float* mean, int B, int T, int D);
void z1_add_bcast(const Ctx& ctx, float* x, const float* v, int B, int T, int D);
void z1_group_rows(const Ctx& ctx, const float* x, float* grp, int B, int T, int Din, int ds);
// SimpleCombiner(src1 [B*T,d1], src2) -> y [B*T,d2]; ub != null: src2 = SimpleUpsample(xd [B,Td,d2], ub [ds,d2])[:T]
void z1_combine(const Ctx& ctx, const float* s1, int d1, const float* s2, int d2, const float* w1, const float* ub, int ds, int B, int T,
                int Td, float* y);
void logfloor_inplace(const Ctx& ctx, float* x, long long n);

}  // namespace k2hip
