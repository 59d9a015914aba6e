/*
 * k2hip_debug.h -- test, tuning and monitoring hooks of libk2hip.so.
 *
 * NOT part of the drop-in boundary (include/k2hip.h): nothing here has a counterpart in
 * K2TransducerAsr's IOfflineProj / IOnlineProj, and a host that replaces the reference's
 * operators never calls these.  They exist so that the parity tests (tests/), the tuning
 * tools (tools/) and a service's monitoring can look inside the engine through the same
 * C ABI instead of through private symbols; every exported `k2hip_debug_*` symbol of the
 * library is declared here (tests/test_abi.py holds the export table to the two headers).
 * Same conventions as k2hip.h: int32 status, message in k2hip_last_error(), host pointers.
 */
#ifndef K2HIP_DEBUG_H
#define K2HIP_DEBUG_H
#include "k2hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* (k2hip_debug_set_switch is declared in k2hip.h: INTEGRATION.md documents the switches.) */

/* ---- search ------------------------------------------------------------------------------------ */
/* one-part repeats of the vocabulary-parallel search since the model was created (K2HIP_ERR_HIP in k2hip.h explains when the
 * engine repeats a search) */
int32_t k2hip_debug_search_retries(k2hip_model_t* model, int32_t* n);
/* the all-contexts decoder table against the decoder routine itself on `n_samples` sampled contexts (plus the start contexts):
 * rows = rows compared, mismatched = rows that are not bit-equal */
int32_t k2hip_debug_decoder_table_check(k2hip_model_t* model, int32_t n_samples, uint32_t seed, int64_t* rows, int64_t* mismatched);
/* Per-frame tap of the modified beam search.  With the switch K2HIP_BEAM_TRACE on, every SYNCHRONOUS batch call under
 * modified_beam_search (and k2hip_beam_search) records, per stream and frame, 2 * beam + 1 int32 words: the `beam` selected
 * candidates in rank order (score desc, flat index asc) as flat indexes `hypothesis slot * vocab_size + token` (-1 where the frame
 * had fewer candidates), their scores as float bits, and the number of hypotheses that survive the frame's merges.
 * trace: [B][Tprime][2 * beam + 1] (NULL only queries the three sizes).  tests/parity.py compares it with the oracle's tap
 * (oracle/k2_oracle_beam.c) to find the first frame at which the two searches part. */
int32_t k2hip_debug_beam_trace(k2hip_model_t* model, int32_t* trace, int64_t cap_words, int32_t* B, int32_t* Tprime, int32_t* beam);

/* Hotword graphs of the streaming search (k2hip_online_stream_set_hotwords, k2hip_beam_stream_set_hotwords): uploads = tables
 * uploaded for this model's streams since it was created, resident = graphs on the device now */
int32_t k2hip_debug_stream_hotword_uploads(k2hip_model_t* model, int32_t* uploads, int32_t* resident);
/* modified beam searches enqueued by this process so far, by kernel instantiation: plain = the unbiased kernels, hotwords = the
 * biased ones (a call in which no stream has a graph must count as plain) */
int32_t k2hip_debug_beam_launch_counts(int64_t* plain, int64_t* hotwords);

/* ---- streaming --------------------------------------------------------------------------------- */
/* mark a stream as if a chunk step over it had failed on the device (k2hip_online_step's poisoning rule, k2hip.h) */
int32_t k2hip_debug_poison_stream(k2hip_online_stream_t* s);
/* does the stream's device mirror of its feature FIFO hold the FIFO right now? */
int32_t k2hip_debug_stream_mirrored(const k2hip_online_stream_t* s, int32_t* ok);

/* ---- GEMM kernels ------------------------------------------------------------------------------ */
/* ONE launch of tile configuration `cfg` (-1: the dispatcher's own choice for the shape; the numbering is csrc/gemm.hip's) on the
 * caller's operands: C = act(A W^T + bias) (+ res).  A [M,K], W [N,K], bias [N] or NULL, res [M, ldo] or NULL, C [M, ldo] row-major
 * f32 in host memory; act = 0 none, 1 SwooshL, 2 SwooshR, 3 tanh, 4 sigmoid, 5 ReLU, 6 DoubleSwish.  glu = 0: ldo = N.
 * glu = 1 / 2: the first `glu_cols` (0 = all N) columns are blocks of 32 = 16 values | their 16 gates and the epilogue writes
 * value * sigmoid(gate) / value * tanh(gate): ldo = glu_cols / 2 + (N - glu_cols).  C is pre-filled with NaNs, so an element the
 * kernel does not write shows.  tests/test_gemm_gpu.py compares the result with a float64 product computed on the host. */
int32_t k2hip_debug_gemm_run(k2hip_model_t* model, const float* A, const float* W, const float* bias, const float* res, float* C,
                             int32_t M, int32_t N, int32_t K, int32_t act, int32_t glu, int32_t glu_cols, int32_t cfg);
/* The fused form of an offline conv module's in_proj + GLU + depthwise conv for B streams of T frames, D channels and K taps (csrc/
 * gemm_plan.cpp glu_dwconv_pipe_entry; host only, no model and no device): *entry = the pipe tile of the one launch (1: 128 x 64,
 * 5: 64 x 64, 8: 128 x 128), or -1 where the two launches run -- a streaming site (streaming != 0), fewer than 256 rows, a GLU GEMM
 * that does not run on one of these tiles or whose tile does not hold a stream, the switch K2HIP_NO_FUSED_CONV
 * (tests/test_conv_fused_plan.py). */
int32_t k2hip_debug_conv_fused_plan(int32_t B, int32_t T, int32_t D, int32_t K, int32_t streaming, int32_t* entry);
/* ---- other encoder kernels ---------------------------------------------------------------------- */
/* ONE launch of the launcher named `op` (csrc/kernels.h: attn_scores_softmax, attn_av_out, attn_av_out_ring, attn_proj_av_out_ring,
 * nonlin_av_out_ring, attn_stream_ring, attn_stream, glu_causal_conv, biasnorm, bypass, biasnorm_bypass, biasnorm_bypass_downsample,
 * downsample, downsample_full, upsample_combine, upsample_combine_downsample, glu_dwconv1d_swoosh, glu_dwconv1d_dswish, dwconv1d_swoosh,
 * dwconv7x7; the Conformer's conformer_qprep, conformer_scores_softmax, conformer_softmax_shift, conformer_softmax_shift_stream,
 * slice_rows, dwconv_valid_dswish; Zipformer v1's z1_pool, z1_attn, z1_glu_conv, z1_norm_bypass, z1_attn_downsample, z1_combine, z1_mean,
 * z1_add_bcast, z1_group_rows; the LSTM's lstm_cell, lstm_cell_rows, lstm_add_frame, lstm_norm_frame, add_inplace, gather_rows,
 * scatter_rows; basicnorm, conv0_pad1_dswish, conv0_nopad_dswish; the kernels around the layers, gemm, gemm_glu_causal_conv and
 * gemm_glu_dwconv1d: see below)
 * on host operands, on the
 * engine's stream.  iargs: the launcher's integer arguments in its own order (a RingRef counts as slot_stride, off; downsample_full's
 * segments put n, ld[n], col1[n], lz_Td, lz_ds, lz_Do in front; long long strides and offsets -- slot_stride, off, avg_off, len_off,
 * ldgx, SY, pstride, lstride, add_inplace's n -- are integer arguments like the ints).  A float argument (`scaling` of conformer_qprep
 * and conformer_scores_softmax) travels in its place among the integer arguments as its IEEE-754 bit pattern, zero-extended: 1.0f is
 * 0x3f800000.  Default arguments are passed explicitly (ldq = 0: rows of 3 D floats / of D floats).  bufs / buf_bytes: its pointer
 * arguments in order (a RingRef as pool, slots, chunks; the segments as src[n], lz_orig, lz_xd, lz_scale), each uploaded whole -- in
 * place operands (x of attn_av_out, the state pool, int arrays) work as they are; NULL or 0 bytes passes a null pointer.  Every buffer
 * sits between two 16 KB guards of 0xff bytes (NaN): a read past either end that reaches the result shows as NaN, and a guard that
 * changed fails the call (K2HIP_ERR_INVALID, naming the buffer).  After the launch the buffers flagged in out_mask (bit k = bufs[k]) are
 * downloaded.  A shape the launcher refuses returns K2HIP_ERR_UNSUPPORTED with nothing launched and nothing downloaded.  Branch
 * switches (K2HIP_ATTN_LONG, K2HIP_DW1D_TT, K2HIP_DW7_TILED, K2HIP_CONFORMER_GEMM_SCORES) go through k2hip_debug_set_switch.
 * tests/test_kernels_gpu.py (Zipformer2) and tests/test_family_kernels_gpu.py (Conformer, Zipformer v1, LSTM) compare each kernel with
 * a float64 reference computed on the host.
 * Two more ops launch the GEMM in every form GemmArgs (csrc/kernels.h) can say (tests/test_gemm_forms_gpu.py):
 *   "gemm": ONE gemm() call.  iargs: GemmArgs' integer and stride fields in their declared order -- M, N, K, lda, ldw, ldc, ldr, act,
 *     act_cols, w_kn, nb0, nb1, sA0, sA1, sW0, sW1, sC0, sC1, sR0, sR1, sBias0, cv_Fout, cv_Tout, cv_Tin, cv_Fin, cv_C, cv_st, cv_sf,
 *     seg_len, seg_stride, res_div, act_after_res, glu, glu_cols, ldm, sM0, sM1, ld_orig (not the tuning fields xcd_panels, dbg, ablate,
 *     and not cf_*: the next op) -- then the cfg force code as k2hip_debug_gemm_run takes it (-1: the dispatcher's choice), res_is_C
 *     (1: the residual is C's own device buffer, the in-place form; no res buffer then), and the offsets in floats of the A, W, res,
 *     C, mul and byp_orig pointers inside their buffers.  bufs: A, W, bias, res, C, skip_if_zero (one int32), mul, byp_orig,
 *     byp_scale, each optional but A, W and C, then a buffer of 5 int32 the hook itself fills with plan_gemm()'s choice for the call:
 *     family (0 register-staged, 1 LDS-DMA, 2 pipe, 3 p16, 4 ring, 5 / 6 / 7 skinny<3> / <6> / <6, 8>), table index, BM, BN, and the
 *     register-staged kernel's addressing mode (0 plain, 1 conv gather, 2 [K,N]).  The hook checks no extent: the caller sizes the
 *     buffers for the addresses its arguments describe.  A K2_REQUIRE of gemm() or a forced plan that does not fit the call is
 *     K2HIP_ERR_UNSUPPORTED.
 *   "gemm_glu_causal_conv": the launcher's arguments in its own order (x, wg, bg, pool, slot_stride, off, slots, wc, bc, ww, bw, sc,
 *     y, B, Tc, D, K), then a buffer of 1 int32 that the hook fills with glu_conv_ring_entry(B, Tc, D, K) (-1: no fused form, and the
 *     call is K2HIP_ERR_UNSUPPORTED with nothing launched).
 *   "gemm_glu_dwconv1d" (tests/test_conv_fused_offline_gpu.py): the first two thirds of an OFFLINE conv module as the layer body runs
 *     them for the shape.  bufs x [B T, D], wg [2 D, D] and bg [2 D] (the "#glu" row-interleaved in_proj: row 32 q + p = value of channel
 *     16 q + p, row 32 q + 16 + p = its gate), wd [K][D], bd [D], y [B T, D] (out), then a buffer of 1 int32 that the hook fills with
 *     k2hip_debug_conv_fused_plan's entry for the shape; ints B, T, D, K.  entry >= 0: ONE launch (gemm_glu_dwconv1d); -1: the two
 *     launches -- the GLU GEMM + dwconv1d_swoosh from 256 rows on, else the plain in_proj (the hook puts the rows back in value | gate
 *     order) + glu_dwconv1d_swoosh.  The switch K2HIP_NO_FUSED_CONV keeps the two launches.
 * The two kernels of the forced alignment (csrc/align.hip, tests/test_align_gpu.py); every stream's plane [T_b][U_b + 1] lies back to
 * back in stream order, T_b = n_frames[b] (a null buffer: Tp), U_b = lens[b]; cells outside the reachable band keep what they held:
 *   "lattice_logprobs": buffers enc [B][Tp][J], n_frames [B] int32, ids (int64, the targets back to back), lens [B] int32, stay, emit
 *     (out); ints B, Tp.  The targets pass the checks of k2hip_transducer_align.
 *   "lattice_dp": buffers n_frames, lens, stay, emit (in), timestamps [B][max_tokens] int32, token_log_probs [B][max_tokens],
 *     scores [B][2] = (total, best) (out); ints B, Tp, max_tokens.  What lies behind a row's first lens[b] entries is unspecified.
 * The CTC forced alignment's device path alone (csrc/ctc_align.hip: gather + lattice; tests/test_ctc_align_gpu.py):
 *   "ctc_lattice": buffers log_probs [R][Tp][V], n_frames [R] int32 (or null), stream_of [H] int32 (or null), ids (int64, the targets
 *     back to back), lens [H] int32, timestamps, end_frames [H][max_tokens] int32, token_log_probs [H][max_tokens], scores [H][2] =
 *     (total, best) (out); ints R, Tp, H, max_tokens.  The arguments pass the checks of k2hip_ctc_align; what lies behind a row's first
 *     lens[h] entries is unspecified.
 * The two forms of Swoosh's softplus (csrc/act.h; tests/test_act_forms_gpu.py):
 *   "act_forms": ints act (1 SwooshL, 2 SwooshR), n; buffers x [n] (in), y_lean [n], y_libm [n] (out).  One plain elementwise
 *     kernel: y_lean = the activation as the GEMM epilogues and the elementwise kernels compute it (softplus_ge1), y_libm = the same
 *     with the library's general log (softplus_libm).  The two must agree bit for bit.
 * The CTC prefix beam search's kernel alone (csrc/ctc_prefix.hip; tests/test_ctc_prefix_gpu.py):
 *   "ctc_prefix_beam": buffers log_probs [R][Tp][V], n_frames [R] int32 (or null), then the outputs of k2hip_ctc_prefix_beam_search --
 *     tokens [R][nbest][max_tokens] int64, timestamps (int32) and token_log_probs of the same shape, n_tokens [R][nbest] int32, n_hyps [R]
 *     int32, scores [R][nbest] -- and flag [1] int32, the search-output block's status word (1: an entry outgrew max_tokens and was not
 *     written); ints R, Tp, V, beam, nbest, max_tokens.  V here is free, not the model's.  The kernel stores straight into the guarded
 *     buffers, so what it does not write keeps the caller's fill.
 *   "ctc_prefix_beam_bias" (tests/test_ctc_prefix_bias_gpu.py): the same kernel's biased instantiation alone.  The nine buffers of
 *     "ctc_prefix_beam", then caller-supplied tables: next [S][V] int32, bonus [S][V], pending [S] (the dense hotword graph; all three or
 *     all null), LM states [S_lm][4] int32 = (arc begin, arc end, back-off state, back-off weight bits), arc_tok / arc_lp / arc_next [A],
 *     uni_lp / uni_next [V] (the scaled sparse LM; all or all null, the arc buffers null when A = 0); ints R, Tp, V, beam, nbest,
 *     max_tokens, S, S_lm, A, start.  V is free.  Before the launch the host checks everything the kernel indexes with -- every next,
 *     arc_next, uni_next and back-off state in range, arc ranges inside [0, A] and ordered, the start state in range -- and fails with
 *     K2HIP_ERR_INVALID otherwise: a bad table cannot fault the device.
 *   "ctc_prefix_resume" (tests/test_ctc_prefix_stream_gpu.py): the same kernel's resume form alone.  Buffers log_probs [B][Tc][V],
 *     n_frames [B] int32 in 1..Tc (or null), in [B][in_ints] -- the caller's in blocks, laid out as kernels.h describes beside
 *     CtcPrefixResumeArgs (csrc/ctc_prefix_layout.h has the offsets) --, out [B][out_ints] and status [1] int32 (1: an in block
 *     contradicts itself); ints B, Tc, V, beam.  V is free.  The in blocks are checked on the host first (n, last tokens, relation
 *     lengths: everything the kernel indexes with); the kernel stores straight into the guarded out buffer.
 *   "ctc_prefix_resume_bias" (tests/test_ctc_prefix_stream_bias_gpu.py): the resume form's biased instantiation alone.  The five buffers
 *     of "ctc_prefix_resume", then side in [B][1 + 3K] = [flags | ctx[K] (float bits) | hs[K] | ls[K]] (flags bit 0: the row runs the
 *     LM; K = beam) and side out [B][5K] = [ctx[K] | hs[K] | ls[K] | fin[K] (float bits) | ord[K]] (csrc/ctc_prefix_layout.h,
 *     CtcPrefixResumeBiasLayout), the nine table buffers of "ctc_prefix_beam_bias" (one set per call) and row_graph [B] int32: 1 = the
 *     row reads the hotword tables, 0 = null tables for that row; ints B, Tc, V, beam, S, S_lm, A, start.  V is free.  The host runs
 *     the table check of "ctc_prefix_beam_bias" and the range checks of the side in blocks (every hs inside the row's graph, every ls
 *     inside the LM where the flag is set, no flag without LM tables, no row_graph without hotword tables) first and fails with
 *     K2HIP_ERR_INVALID; the kernel stores straight into the guarded out and side out buffers.
 * The kernels around the encoder layers (tests/test_outer_kernels_gpu.py; cases and references in tests/outer_kernels.py), arguments in
 * the launcher's own order as above, a bool as an int:
 *   offline front end: "pad_logfloor" (bufs packed, d_off int64 [B], d_len int64 [B], out; ints B, L), "pad_logfloor_dense" (bufs feats,
 *     out; ints n_each, B, L), "conv0_swoosh" (as conv0_nopad_dswish), and "gather_samples": the launcher takes a device table of source
 *     pointers, which the hook builds from float offsets into ONE uploaded samples buffer -- ints B, nmax, off[0 .. B); bufs samples,
 *     n (int64 [B]), dst [B][nmax].  The samples buffer starts on a 256-byte boundary, so an offset that is a multiple of 4 puts a
 *     source on a 16-byte boundary and any other offset off it.
 *   streaming state movers (csrc/online.hip): "convnext_cat" (bufs a3, pool, slots, cat, byp; ints slot_stride, embed_off, B, T3, Tc, F,
 *     C), "cat_shift" (bufs pool, slots, newrows, cat; ints slot_stride, off, ldn, B, L, Tc, width, tanh_gated), "cat_keep" (the same
 *     with keep_back last), "fifo_append" (bufs fifo, src, slots, pos; ints cap, feat, G, nf), "fifo_gather" (bufs fifo, slots, head, x;
 *     ints cap, feat, B, T), "zero_floats" and "logfloor_inplace" (one buffer; int n).
 *   small elementwise kernels: "glu_sigmoid" (bufs x, y; ints M, D), "tanh_gate" (bufs x, y; ints M, Hc), "convert_channels" (bufs x, y;
 *     ints M, Din, Dout), "copy_cols" (bufs x, y; ints ldx, xcol0, ldy, ycol0, M, n), "tanh_add" (bufs enc, dec, y; ints dec_stride, N, J).
 *   search tail (csrc/greedy.hip): "argmax_rows" and "argmax_first_rows" (bufs logits, tok int32 [N]; ints ld, N, V), "log_softmax_rows"
 *     (one buffer, in place; ints M, V), "ctc_collapse" (bufs tok int32 [B][Tp], frame_off int32 [B] or null, tokens int64
 *     [B][max_tokens], timestamps, n_tokens, trail, any, overflow (int32; the kernel only ever raises overflow: pass it as 0); ints B, Tp,
 *     max_tokens), "first_emit_frame" (bufs tok int32 [B][Tp], t0 int32 [1]; ints B, Tp, skip1).
 * One op launches nothing (tests/test_search_ties_gpu.py):
 *   "greedy_screen_counts": no int arguments, one buffer of 2 int64 that the hook fills (whatever out_mask says) with the model's
 *     counters since it was created: [0] rounds of the persistent large-vocabulary greedy search (csrc/greedy.hip k_greedy) that its
 *     f16 screen decided, [1] rounds that ran the f32 passes instead (non-finite screen values, more than 64 candidates, or a slab
 *     too wide for the screen) -- one count per round and column slab of a stream.  They only move while the switch
 *     K2HIP_SCREEN_COUNT is on; a model loaded with K2HIP_SCREEN_MIN_V=0, a small vocabulary and the K2HIP_SEARCH_ROUNDS=1 form
 *     never count.  Call it with no pipelined search in flight. */
int32_t k2hip_debug_op_run(k2hip_model_t* model, const char* op, const int64_t* iargs, int32_t n_iargs, void* const* bufs,
                           const int64_t* buf_bytes, int32_t n_bufs, uint32_t out_mask);
/* The two kernels of the keyword spotter (csrc/kws.hip; tests/test_kws_gpu.py) through k2hip_debug_op_run:
 *   "trie_logprobs": bufs enc [B][Tp][J], n_frames [B] int32 (or null = Tp), the keywords' ids int64 back to back, lens [P] int32,
 *     thresholds [P], stay, emit (out: every stream's plane [T_b][S], back to back; all streams walk the one graph, which the hook builds
 *     and makes resident for the call); ints B, Tp, P.
 *   "trie_dp": bufs n_frames [B] int32 (or null), parent, depth, kw [S] int32, bar [S] (taken as given), stay, emit (in, laid out as
 *     above), a [B][S], start [B][S] int32 (in / out: the carried blocks of csrc/kws_ref.h), ev_keyword [B][Tp] int64, ev_start, ev_end
 *     [B][Tp] int32, ev_sum [B][Tp], n_events [B] int32 (out; row b holds n_events[b] events); ints B, Tp, S. */

/* ---- keyword spotting (k2hip.h "Keyword spotting") ---------------------------------------------- */
/* the carried block of a keyword stream: a [S] and start [S] (S = k2hip_keywords_num_states of its graph).  State 0 is the root:
 * a = 0, start = the stream's frame count.  A state without a token holds (-inf, -1). */
int32_t k2hip_debug_kws_stream_get_state(const k2hip_kws_stream_t* s, float* a, int32_t* start, int32_t cap);
/* the graph's tables, each [S] (any may be NULL): what tests/test_kws.py holds against its Python restatement */
int32_t k2hip_debug_keywords_get_tables(const k2hip_keywords_t* kw, int32_t* parent, int32_t* tok, int32_t* depth, int32_t* keyword, float* bar,
                                        int32_t cap);
/* the float32 host reference of the token passing (csrc/kws_ref.h), no GPU: one stream, planes stay / emit [T][S], the carried block
 * a / start [S] updated in place, events into ev_* [cap] (K2HIP_ERR_CAPACITY beyond), *n_events their number */
int32_t k2hip_debug_kws_ref_dp(const int32_t* parent, const int32_t* depth, const int32_t* keyword, const float* bar, int32_t S, const float* stay,
                               const float* emit, int32_t T, float* a, int32_t* start, int32_t* ev_keyword, int32_t* ev_start, int32_t* ev_end,
                               float* ev_sum, int32_t cap, int32_t* n_events);

/* ---- keyword spotting for CTC models (k2hip.h "Keyword spotting for CTC models") ----------------- */
/* the carried block of a CTC keyword stream: v [2][S] and st [2][S] (plane 0 = n, plane 1 = b; S = k2hip_keywords_num_states of its
 * graph; cap counts cells, 2 * S).  n of the root: (0, the stream's frame count); b of the root: (-inf, hold). */
int32_t k2hip_debug_ctc_kws_stream_get_state(const k2hip_ctc_kws_stream_t* s, float* v, int32_t* st, int32_t cap);
/* the float32 host reference of the token passing (csrc/ctc_kws_ref.h), no GPU: one stream, log_probs [T][V], the tables each [S] (bar
 * as given; rc(s) = the root's child whose token is tok(s), or -1), the carried block v / st [2][S] updated in place, events into ev_*
 * [cap] (K2HIP_ERR_CAPACITY beyond), *n_events their number */
int32_t k2hip_debug_ctc_kws_ref_dp(const int32_t* parent, const int32_t* tok, const int32_t* depth, const int32_t* keyword, const float* bar,
                                   const int32_t* rc, int32_t S, const float* log_probs, int32_t V, int32_t T, float* v, int32_t* st,
                                   int32_t* ev_keyword, int32_t* ev_start, int32_t* ev_end, float* ev_sum, int32_t cap, int32_t* n_events);
/* The spotter's kernel (csrc/ctc_kws.hip; tests/test_ctc_kws_gpu.py) through k2hip_debug_op_run on a CTC model:
 *   "ctc_trie_dp": bufs log_probs [B][Tp][V], n_frames [B] int32 (or null = Tp), graph_of [B] int32 (or null = graph 0), the G graphs'
 *     tables back to back, each [parent | tok | depth | kw | bar | rc] x [S_g] words (bar taken as given), n_states [G] int32, v, st (in /
 *     out: every stream's carried block [2][S], back to back), ev_keyword [B][Tp] int64, ev_start, ev_end [B][Tp] int32, ev_sum [B][Tp],
 *     n_events [B] int32 (out; row b holds n_events[b] events); ints B, Tp, G, V (the log-probs' width: any, not the model's). */

/* ---- input at other sample rates (k2hip.h "Input at other sample rates"; tests/test_resample.py, test_resample_gpu.py) ---------- */
/* the plan of csrc/resample_plan.h for in_rate -> out_rate, host only, no model: *iu, *ou, *max_taps, then (each may be NULL; all NULL =
 * the sizes alone) first [ou], ntaps [ou] and the float32 weights w [ou][max_taps], rows zero-filled behind ntaps[p].  K2HIP_ERR_CAPACITY
 * when cap_phases < ou or cap_w < ou * max_taps; the refusals of k2hip.h otherwise. */
int32_t k2hip_debug_resample_plan(int32_t in_rate, int32_t out_rate, int32_t* iu, int32_t* ou, int32_t* max_taps, int32_t* first, int32_t* ntaps,
                                  float* w, int32_t cap_phases, int64_t cap_w);
/* outputs that exist after n_in_total input samples (-1 on error) */
int64_t k2hip_debug_resample_num_out(int32_t in_rate, int32_t out_rate, int64_t n_in_total);
/* the float32 host reference (csrc/resample_ref.h), no GPU: one push of n samples x into a stream whose carried block is tail
 * [*n_tail] (the input samples [*n_in - *n_tail, *n_in)) and the counts *n_in / *n_out, all updated in place (a fresh stream: 0, 0, 0);
 * the outputs the push completes go to out, *n_written their number.  K2HIP_ERR_CAPACITY beyond cap / tail_cap. */
int32_t k2hip_debug_resample_ref(int32_t in_rate, int32_t out_rate, float* tail, int64_t* n_tail, int64_t tail_cap, int64_t* n_in, int64_t* n_out,
                                 const float* x, int64_t n, float* out, int64_t cap, int64_t* n_written);
/* how many plans the model has built: one per input rate other than its own that an entry has named */
int32_t k2hip_debug_resample_plans(k2hip_model_t* model, int32_t* n);
/* The kernel alone (csrc/resample.hip) through k2hip_debug_op_run:
 *   "resample_gather": ints B, n_dst_rows, nmax, then per row (in_rate, out_rate, off_head, n_head, off_tail, n_tail, x0, k0, n_out,
 *     dst_row); bufs samples, dst [n_dst_rows][nmax] (out).  Row b reads the two pieces samples[off_head .. + n_head) ;
 *     samples[off_tail .. + n_tail), the first float being input sample x0 of its stream, and writes outputs k0 .. k0 + n_out of the plan
 *     in_rate -> out_rate, then zeros up to nmax, into row dst_row.  in_rate = 0: a pass-through row, the pieces copied and zero-filled.
 *     The samples buffer starts on a 256-byte boundary, so an offset that is no multiple of 4 puts a piece off the 16-byte boundary.
 *     The launcher checks on the host that no row reads outside its pieces or writes outside its row: K2HIP_ERR_UNSUPPORTED. */

/* ---- voice activity detection (k2hip.h "Voice activity detection and long recordings"; tests/test_vad.py, test_vad_gpu.py) ------- */
/* host only, no model and no GPU: the config rules for feature rows of num_bins floats; the default band of a filterbank; the long
 * entry's packing rule over n segment lengths in frames (batch_of [n]) */
int32_t k2hip_debug_vad_check_config(const k2hip_vad_config* cfg, int32_t num_bins);
int32_t k2hip_debug_vad_default_config(int32_t sample_rate, int32_t num_bins, float low_freq, float high_freq, k2hip_vad_config* cfg);
int32_t k2hip_debug_vad_pack(const int64_t* len, int32_t n, int32_t max_batch, int64_t max_batch_frames, int32_t* batch_of);
/* a stream without a model, for rows of num_bins floats: every k2hip_vad_stream_* entry works on it, the accept entries do not */
int32_t k2hip_debug_vad_ref_stream_create(int32_t num_bins, const k2hip_vad_config* cfg, k2hip_vad_stream_t** out);
/* the float32 host reference (csrc/vad_ref.h), no GPU: n rows (num_bins or the model's feature_dim floats each) pushed into the stream's
 * carried state, on a stream of either kind; the taps m, n, d (each may be NULL) get n entries */
int32_t k2hip_debug_vad_ref_push(k2hip_vad_stream_t* s, const float* feats, int64_t n, float* tap_m, float* tap_n, uint8_t* tap_d);
/* the taps of the model's last accept call (or of its last k2hip_offline_recognize_long): stream b's frames of that call.  *n_frames is
 * set; K2HIP_ERR_CAPACITY when cap is short */
int32_t k2hip_debug_vad_taps(k2hip_model_t* model, int32_t b, float* m, float* n, uint8_t* d, int64_t cap, int64_t* n_frames);
/* host milliseconds of the last k2hip_offline_recognize_long by leg: fbank (with the upload), the detector, the batches */
int32_t k2hip_debug_long_timing(k2hip_model_t* model, double* ms3);

/* ---- neural LM rescoring (k2hip.h "Neural LM rescoring"; tests/test_rnn_lm.py, test_rnn_lm_gpu.py, tools/rnn_lm_bench.py) ---------- */
/* host only, no model and no GPU: the row plan of a scoring call (csrc/rnn_lm_plan.h) over Hn hypotheses, hidden width H and a cap of
 * gx_cap_floats floats per time block (<= 0: the default).  order [Hn], active [cap_T], base [cap_T + 1], block [cap_T + 1]; *T and
 * *n_blocks are set; K2HIP_ERR_CAPACITY when cap_T is short of T. */
int32_t k2hip_debug_rnn_lm_plan(const int64_t* offsets, int32_t Hn, int32_t with_eos, int32_t H, int64_t gx_cap_floats, int32_t* order,
                                int32_t* active, int64_t* base, int32_t* block, int32_t cap_T, int32_t* T, int32_t* n_blocks);
/* scoring calls that reached the device since the model was created; the time blocks of the last one */
int32_t k2hip_debug_rnn_lm_stats(k2hip_model_t* model, int64_t* device_calls, int32_t* last_blocks);
/* on != 0: every scoring call brackets its legs with events and waits for them; ms4 (may be NULL) gets the last call's milliseconds by
 * leg: embed, GX, steps, score */
int32_t k2hip_debug_rnn_lm_timing(k2hip_model_t* model, int32_t on, double* ms4);
/* milliseconds per recurrent step of `rows` rows at hidden width H on pseudo-random operands, `iters` launches between two events: the
 * fused step kernel, and the step composed from the GEMM launcher and the cell kernel as the LSTM encoder's lstm_layer does */
int32_t k2hip_debug_rnn_lm_step_bench(k2hip_model_t* model, int32_t rows, int32_t H, int32_t iters, float* fused_ms, float* composed_ms);
/* k2hip_debug_op_run ops, each ONE launch on the caller's buffers:
 *   "rnn_lm_embed"  ints R, E; bufs emb [V][E], ids [R] (int32, in [0,V): not checked), x0 [R][E] (out)
 *   "rnn_lm_step"   ints a, H, first (1: h = 0, h_prev is not read); bufs h_prev [a][H], whh_kn [H][4H], gx [rows][4H], c [rows][H]
 *                   (in / out), h_out [rows][H] (out): rows >= a of c and h_out stay as they were
 *   "rnn_lm_score"  ints R, H, V, Vp; bufs y [R][H], out_kn [H][Vp], out_b [V], target [R] (int32), lp [R] (out) */

/* ---- neural LM shallow fusion (k2hip.h "Neural LM shallow fusion"; tests/test_rnn_lm_fusion_gpu.py, tools/rnn_lm_fusion_bench.py) ---- */
/* searches: fused searches enqueued since the process started (the third counter beside k2hip_debug_beam_launch_counts: a fused
 * search moves neither of those); swept / idle: per-layer LM launches of this model's attached LM that read their weights / that only
 * moved state because no slot of the batch appended a token on their frame (counted on the device; 0 without an LM).  Each may be NULL. */
int32_t k2hip_debug_rnn_lm_fusion_stats(k2hip_model_t* model, int64_t* searches, int64_t* swept, int64_t* idle);
/* milliseconds per k_nlm_advance launch of `rows` rows that all append, input and hidden width H (2 H products per gate; the rescoring
 * step of k2hip_debug_rnn_lm_step_bench sums H), a scattered parent map, pseudo-random operands, `iters` launches between two events */
int32_t k2hip_debug_nlm_advance_bench(k2hip_model_t* model, int32_t rows, int32_t H, int32_t iters, float* ms);
/* k2hip_debug_op_run ops:
 *   "nlm_advance"  ONE launch.  ints M, in, H, use_emb, V, live (-1: no flag; else the device flag is set to it first); bufs wcat (the
 *                  layer's panels: kernels.h RnnLmDev::wcat), bias [4H], x (emb [V][in] when use_emb, else rows [M][in]), h_par [M][H],
 *                  c_par [M][H], h_out [M][H] (out), c_out [M][H] (out), par [M] (int32), tok [M] (int32, -1: nothing appended),
 *                  flag [1] (int32), work [2] (int64 counters, in / out)
 *   "nlm_rows"     the GEMM launcher + one launch.  ints M, H, V, live; bufs h [M][H], w_out [V][H], out_b [V], q_par [M][V],
 *                  q_out [M][V] (out), par [M], tok [M], flag [1] */

/* ---- neural LM shallow fusion in the streaming search (k2hip.h; tests/test_rnn_lm_stream_fusion_gpu.py) ---- */
/* chunk_calls: fused chunk calls (k2hip_beam_search_chunk / k2hip_online_step ticks) enqueued since the process started -- they move
 * neither k2hip_debug_beam_launch_counts nor the counters of k2hip_debug_rnn_lm_fusion_stats; live_blocks: state blocks this model's
 * streams hold; pool_bytes: device memory of the model's block pool (held and spare blocks).  Each may be NULL. */
int32_t k2hip_debug_rnn_lm_stream_fusion_stats(k2hip_model_t* model, int64_t* chunk_calls, int64_t* live_blocks, int64_t* pool_bytes);
/* k2hip_debug_op_run ops (the block layout: csrc/rnn_lm_stream_pool.h NlmStreamLayout -- per half states [K][L][2][H], rows [K][V],
 * rounded up to 4 floats; a block is two halves):
 *   "nlm_load_streams"   ints B, K, L, H, V; bufs blocks [B][block], cur [B] (int32: the half that is read, -1: a stream without a state),
 *                        nh [B] (int32: live slots), h0 [L][H], c0 [L][H], q0 [V], h [L][B K][H] (out), c (out), q [B K][V] (out),
 *                        io [B] x 16 bytes (scratch: the block-pointer table)
 *   "nlm_store_streams"  ints B, K, L, H, V; bufs blocks (in / out), cur [B] (the half NOT written; -1: half 0 is written), h, c, q, io */

/* ---- GEMM tuning ------------------------------------------------------------------------------- */
/* time `iters` launches of a shape / configuration on pseudo-random operands (tools/gemm_lab.py, gemm_tune.py) */
int32_t k2hip_debug_gemm(k2hip_model_t* model, int32_t M, int32_t N, int32_t K, int32_t act, int32_t with_res, int32_t cfg,
                         int32_t iters, float* ms);
/* the same, and max_err = largest |difference| from the register-staged kernel on the same operands (a GPU-vs-GPU figure for
 * the tuning tools; the parity test is k2hip_debug_gemm_run against the host) */
int32_t k2hip_debug_gemm_check(k2hip_model_t* model, int32_t M, int32_t N, int32_t K, int32_t act, int32_t with_res, int32_t cfg,
                               int32_t iters, float* ms, float* max_err);
/* ONE launch with in-kernel s_memtime stamps: out [n_wg][n_waves][64] (tools/gemm_dma_trace.py) */
int32_t k2hip_debug_gemm_trace(k2hip_model_t* model, int32_t M, int32_t N, int32_t K, int32_t act, int32_t with_res, int32_t cfg,
                               unsigned long long* out, int64_t cap, int32_t* n_wg, int32_t* n_waves);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* K2HIP_DEBUG_H */
