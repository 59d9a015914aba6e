/*
 * k2hip.h -- C ABI of libk2hip.so, the MI355X (gfx950) engine behind
 * K2TransducerAsr's IOfflineProj / IOnlineProj operator boundary.
 *
 * Every entry point replaces one reference interface (file:line relative to the
 * reference repo manyeyes/K2TransducerAsr @ 2025-09-19).  The C# side binds them
 * with [DllImport("k2hip")] (csharp/OfflineProjOfHip.cs).
 *
 * Conventions
 *   - every function returns int32 status: 0 = ok, < 0 = error; the message is
 *     in k2hip_last_error() (thread-local).  Nothing throws across the ABI.
 *     (replaces `throw new Exception("EncoderProj failed", ex)`,
 *      OfflineProjOfTransducer.cs:87-90; "Offline recognition failed",
 *      OfflineRecognizer.cs:183-186,299-302)
 *   - all buffers are caller-owned, row-major, f32 / i64 exactly as the reference
 *     marshals them to ONNXRuntime; pointers are host pointers unless the name
 *     says `_dev`.
 *   - one k2hip_model_t = one GPU + one HIP stream; calls on the same handle are
 *     serialised by an internal mutex, different handles run concurrently.
 *   - there is NO CPU fallback: every compute entry point needs a gfx950 device
 *     and fails with K2HIP_ERR_NO_DEVICE otherwise.
 *   - memory: a handle holds, on its device, the model's weights (the .k2w file's size), a grow-only arena per pipeline slot
 *     (~1.1 GB each for 32 x 10 s of zipformer2-large), the streaming state pool (1.85 MB per stream for the medium model) and --
 *     for vocabularies up to ~700 -- the decoder's output for EVERY two-token context, (V + 1) * V * joiner_dim floats (0.5 GB at
 *     V = 500, J = 512), built inside k2hip_model_create (~3 ms of GPU time).  N handles on one GPU hold N copies.  The environment
 *     variable K2HIP_DECODER_TABLE_MB caps the table (default 1024; 0 = never build it: the searches then run the decoder after
 *     every emission, ~1.7x slower per search, same tokens).
 */
#ifndef K2HIP_H
#define K2HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */
#endif

#define K2HIP_OK 0
#define K2HIP_ERR_INVALID (-1)   /* bad argument / shape */
#define K2HIP_ERR_IO (-2)        /* weight file missing or malformed */
#define K2HIP_ERR_NO_DEVICE (-3) /* no usable HIP device */
#define K2HIP_ERR_HIP (-4)       /* a HIP runtime call failed.  Also: the greedy search's vocabulary-parallel exchange timed out TWICE -- its
                                  * workgroups wait for each other and need to be resident together; on a timeout (a GPU shared with other
                                  * processes / models) the library repeats the search with one workgroup per stream, which waits for nobody,
                                  * so a call under load gets slower instead of failing; only if that repeat also reports a timeout (it cannot,
                                  * short of a device fault) does the call return this code */
#define K2HIP_ERR_CAPACITY (-5)  /* caller buffer too small */
#define K2HIP_ERR_UNSUPPORTED (-6)

typedef struct k2hip_model k2hip_model_t;
typedef struct k2hip_offline_stream k2hip_offline_stream_t;
typedef struct k2hip_online_stream k2hip_online_stream_t;
typedef struct k2hip_beam_stream k2hip_beam_stream_t;
typedef struct k2hip_tokens k2hip_tokens_t;
typedef struct k2hip_hotwords k2hip_hotwords_t;
typedef struct k2hip_ngram_lm k2hip_ngram_lm_t;
typedef struct k2hip_keywords k2hip_keywords_t;
typedef struct k2hip_kws_stream k2hip_kws_stream_t;
typedef struct k2hip_ctc_kws_stream k2hip_ctc_kws_stream_t;

/* Fixed ids of the reference: OfflineModel.cs:18-20. */
#define K2HIP_BLANK_ID 0
#define K2HIP_SOS_EOS_ID 1
#define K2HIP_UNK_ID 2

typedef struct k2hip_model_info {
    int32_t vocab_size;   /* decoder metadata "vocab_size"   OfflineModel.cs:36-38 */
    int32_t context_size; /* decoder metadata "context_size" OfflineModel.cs:33-35 */
    int32_t joiner_dim;   /* joiner metadata "joiner_dim"    OfflineModel.cs:43-45 */
    int32_t feature_dim;  /* OfflineModel.FeatureDim         OfflineModel.cs:21    */
    int32_t sample_rate;
    int32_t num_stacks;
    int32_t device;
    int32_t reserved; /* encoder output width: joiner_dim, or vocab_size for a zipformer2ctc model (log_probs) */
} k2hip_model_info;

/* Per-call stage timings of the last fused call, measured with HIP events on the
 * model's stream (replaces the reference's DateTime.Now.Ticks RTF print,
 * K2TransducerAsr.Examples/OfflineRecognizer.cs:144,184-189). */
typedef struct k2hip_timing {
    float total_ms;
    float fbank_ms;
    float pad_ms;
    float encoder_ms; /* embed + stacks + proj */
    float greedy_ms;
    float d2h_ms;
    /* GEMM accounting, filled only when instrumentation is enabled with
     * k2hip_set_instrument(model, 1): summed HIP-event duration of every launch
     * of the fp32 MFMA GEMM kernel in the last call, their count and their
     * algorithmic FLOPs (2*M*N*K per launch). */
    float gemm_ms;
    int32_t gemm_launches;
    double gemm_flops;
    double total_flops; /* all matrix work incl. attention/conv (2 FLOP per MAC) */
} k2hip_timing;

/* ---- library ---------------------------------------------------------------- */
const char* k2hip_version(void);
const char* k2hip_last_error(void);
/* number of visible HIP devices (0 if none); never fails */
int32_t k2hip_device_count(void);

/* ---- model: replaces OfflineModel ctor + 3x initModel (OfflineModel.cs:23-73,
 * 84-118).  `weights_path` is a .k2w container holding the ONNX custom-metadata
 * map and all initializers; `overrides` is NULL or "key=value;key=value" applied on
 * top of that map (same keys the reference reads: OfflineModel.cs:31-72,
 * OnlineModel.cs:38-166). A missing file is an error here (the reference returns
 * a null session and fails later with a NullReferenceException, :86-89). */
int32_t k2hip_model_create(const char* weights_path, const char* overrides, int32_t device, k2hip_model_t** out);
int32_t k2hip_model_destroy(k2hip_model_t* model);
/* Device selection through the reference's UNCHANGED constructors (OfflineRecognizer.cs:27-28, OnlineRecognizer.cs:18-19 take file
 * paths and no device): a model spec is "path.k2w" (device 0) or "path.k2w@N" (device N, decimal; the suffix is only split off when
 * what follows the LAST '@' is all digits).  path gets the spec without the suffix (NUL terminated, cap bytes), device the number.
 * Pure string work: no file access, no GPU.  csharp/K2Hip.cs (SplitSpec) implements the same rule in managed code -- it has to
 * answer for ONNX paths on installations without this library -- and tests/native/multi_handle_host.c names its handles this way. */
int32_t k2hip_parse_model_spec(const char* spec, char* path, int32_t cap, int32_t* device);
/* k2hip_model_create on a spec: the container of `spec` on the device it names */
int32_t k2hip_model_create_spec(const char* spec, const char* overrides, k2hip_model_t** out);
int32_t k2hip_model_get_info(const k2hip_model_t* model, k2hip_model_info* info);
/* CustomMetadataMap[key] -> buf (NUL terminated); K2HIP_ERR_INVALID if absent */
int32_t k2hip_model_meta(const k2hip_model_t* model, const char* key, char* buf, int32_t cap);
int32_t k2hip_set_instrument(k2hip_model_t* model, int32_t on);
/* per-launch table of the last instrumented call: rows of 8 floats (M, N, K, batch, act, has_residual, kind, microseconds);
 * kind & 3: 0 plain, 1 conv gather, 2 [K,N] operand; +16 LDS-DMA kernel, +32 skinny kernel, +64 ring kernel, +128 pipelined kernel
 * with its tile in the bits above (BM / 32 in bits 8-11, BN / 32 in bits 12-15; + 2^20: its 16x16x4-tile form).  rows == NULL only queries n_rows. */
int32_t k2hip_get_gemm_profile(k2hip_model_t* model, float* rows, int32_t cap_rows, int32_t* n_rows);
int32_t k2hip_get_timing(const k2hip_model_t* model, k2hip_timing* timing);

/* ---- F1: WavFrontend.GetFbank (WavFrontend.cs:32-36 -> SpeechFeatures.OnlineFbank)
 * samples: f32 in [-1,1]; feats: [n_frames, feature_dim] frame-major.  One-shot
 * (snip_edges) framing of exactly these samples. */
int64_t k2hip_fbank_num_frames(const k2hip_model_t* model, int64_t n_samples);
int32_t k2hip_fbank(k2hip_model_t* model, const float* samples, int64_t n_samples, float* feats, int64_t cap_frames,
                    int64_t* n_frames);

/* ---- F3: PadHelper.PadSequence(List<OfflineInputEntity>) (PadHelper.cs:14-60):
 * right-pad to max+80*tail_frames floats, then every 0.0 -> -23.025850929940457f.
 * out: [B, padded_len]. Runs on the device (the fused entries never call this
 * separately; it is exported so the quirk can be parity-tested on its own). */
int32_t k2hip_pad_sequence(k2hip_model_t* model, const float* const* speech, const int64_t* n_floats, int32_t B,
                           int32_t tail_frames, float* out, int64_t cap_floats, int64_t* padded_len);

/* ---- F4: IOfflineProj.EncoderProj body after padding
 * (OfflineProjOfTransducer.cs:52-85): x [B,T,feature_dim] f32, x_lens [B] i64 (the
 * reference always passes T for every row, :66-70; values are ignored exactly as
 * the reference's loop ignores encoder_out_lens) -> enc_out [B,T',joiner_dim],
 * enc_out_lens [B] (may be NULL), *Tprime. */
int32_t k2hip_encoder_out_frames(const k2hip_model_t* model, int32_t T);
int32_t k2hip_offline_encoder(k2hip_model_t* model, const float* x, const int64_t* x_lens, int32_t B, int32_t T,
                              float* enc_out, int64_t cap_floats, int64_t* enc_out_lens, int32_t* Tprime);
/* debug tap for layer-level parity: tap 0 = encoder_embed out [B,T50,D0];
 * 1+i = stack i out [B,T50,D_i]; 100 = full-dim out [B,T50,Dmax]. */
int32_t k2hip_offline_encoder_tap(k2hip_model_t* model, const float* x, int32_t B, int32_t T, int32_t tap, float* out,
                                  int64_t cap_floats, int64_t* n_floats);

/* ---- F5: IOfflineProj.DecoderProj (OfflineProjOfTransducer.cs:93-123):
 * y [N, context_size] i64 (id < 0 -> zero embedding, used at utterance start,
 * OfflineRecognizer.cs:105) -> dec_out [N, joiner_dim].  y == NULL means
 * [-1, blank] x N (:97-110). */
int32_t k2hip_decoder(k2hip_model_t* model, const int64_t* y, int32_t N, float* dec_out);

/* ---- F6: IOfflineProj.JoinerProj (OfflineProjOfTransducer.cs:125-152):
 * enc [N,J], dec [N,J] -> logits [N, vocab]. */
int32_t k2hip_joiner(k2hip_model_t* model, const float* enc, const float* dec, int32_t N, float* logits);

/* ---- F7 on a precomputed encoder_out: the greedy loops alone.
 * k2hip_greedy_batch  = OfflineRecognizer.ForwardBatchGreedySearch :202-296
 * k2hip_greedy_single = OfflineRecognizer.ForwardGreedySearch      :103-181
 * enc_out [B,T',J] (B = 1 for single).  tokens/timestamps [B, max_tokens] hold the
 * emitted symbols only (the reference's `Tokens` additionally starts with 2*B
 * blanks in the batch path, :250-258, or [-1, blank] in the single path,
 * :115-117; the C# shim re-adds that prefix).  timestamps are 25 Hz frame indices. */
int32_t k2hip_greedy_batch(k2hip_model_t* model, const float* enc_out, int32_t B, int32_t Tprime, int64_t* tokens,
                           int32_t* timestamps, int32_t* n_tokens, int32_t max_tokens);
int32_t k2hip_greedy_single(k2hip_model_t* model, const float* enc_out, int32_t Tprime, int64_t* tokens,
                            int32_t* timestamps, int32_t* n_tokens, int32_t max_tokens);

/* ---- fused hot path: the body of the ForwardBatchOffline delegate
 * (OfflineRecognizer.cs:11,58,189-303): pad (F3) + encoder (F4) + greedy (F7) in
 * one call, one host->device and one device->host crossing.
 * feats[b]: [n_floats[b]] = per-stream OfflineInputEntity.Speech. */
int32_t k2hip_offline_greedy(k2hip_model_t* model, const float* const* feats, const int64_t* n_floats, int32_t B,
                             int64_t* tokens, int32_t* timestamps, int32_t* n_tokens, int32_t max_tokens);
/* ... the ForwardOffline delegate (single stream, :10,57,93-187) */
int32_t k2hip_offline_greedy_single(k2hip_model_t* model, const float* feats, int64_t n_floats, int64_t* tokens,
                                    int32_t* timestamps, int32_t* n_tokens, int32_t max_tokens);
/* ... plus F1: raw samples in (OfflineStream.AddSamples + GetResults). */
int32_t k2hip_offline_greedy_from_samples(k2hip_model_t* model, const float* const* samples, const int64_t* n_samples,
                                          int32_t B, int64_t* tokens, int32_t* timestamps, int32_t* n_tokens,
                                          int32_t max_tokens);
/* Same, with the samples already resident in this model's GPU memory
 * (samples_dev: [B, n_samples_each] contiguous device buffer).  This is the
 * benchmark entry: the timed region starts with inputs in HBM. */
int32_t k2hip_offline_greedy_from_samples_dev(k2hip_model_t* model, const float* samples_dev, int64_t n_samples_each,
                                              int32_t B, int64_t* tokens, int32_t* timestamps, int32_t* n_tokens,
                                              int32_t max_tokens);

/* Pipelined form of the same call, for throughput serving: submit() enqueues the batch and
 * returns a ticket, wait() blocks until THAT batch's tokens are in host memory.  Up to
 * K2HIP_MAX_BATCHES_IN_FLIGHT batches may be in flight: with two, the greedy loop of batch i
 * (latency-bound, a few dozen workgroups) overlaps the encoder of batch i+1 on a second HIP stream; the
 * third is for the modified beam search (k2hip_set_beam), whose per-frame launches take longer
 * than an encoder pass once they share the GPU with one -- the searches of batches i and i+1
 * then run beside the encoder of batch i+2.  Results are identical to the
 * synchronous call (the reference is synchronous: GetResults returns when the batch is done,
 * OfflineRecognizer.cs:85-91; a host that wants that simply calls wait right after submit). */
#define K2HIP_MAX_BATCHES_IN_FLIGHT 3
int32_t k2hip_offline_submit_samples_dev(k2hip_model_t* model, const float* samples_dev, int64_t n_samples_each,
                                         int32_t B, int32_t max_tokens, int32_t* ticket);
int32_t k2hip_offline_wait(k2hip_model_t* model, int32_t ticket, int64_t* tokens, int32_t* timestamps,
                           int32_t* n_tokens);
/* The same with the samples still in HOST memory ([B, n_samples_each] f32), as the reference's caller holds them
 * (K2TransducerAsr.Examples/OfflineRecognizer.cs:164-171): the host-to-device copy is part of the pipeline -- it runs
 * on its own HIP stream under the previous batch's encoder.  The buffer must stay valid and unchanged until
 * k2hip_offline_wait returns for this ticket.  For the copy to be asynchronous it must be page-locked:
 * k2hip_host_alloc / k2hip_host_free hand out such memory (a managed host pins its float[] and registers it, or copies
 * into one of these). */
int32_t k2hip_offline_submit_samples(k2hip_model_t* model, const float* samples_host, int64_t n_samples_each,
                                     int32_t B, int32_t max_tokens, int32_t* ticket);
int32_t k2hip_host_alloc(k2hip_model_t* model, int64_t bytes, void** host_ptr);
int32_t k2hip_host_free(k2hip_model_t* model, void* host_ptr);

/* Development switches (INTEGRATION.md lists them): K2HIP_* environment variables select alternative kernels for the same
 * math or tuning variants.  They are read ONCE, when the first model of the process is created; this call flips one afterwards
 * (the parity tests compare both paths inside one process with it).  Not part of the reference's surface. */
int32_t k2hip_debug_set_switch(const char* env_name, int32_t value);

/* device memory helpers for the benchmark / host runtimes without a HIP binding */
int32_t k2hip_device_alloc(k2hip_model_t* model, int64_t bytes, void** dev_ptr);
int32_t k2hip_device_free(k2hip_model_t* model, void* dev_ptr);
int32_t k2hip_device_upload(k2hip_model_t* model, void* dev_dst, const void* host_src, int64_t bytes);
int32_t k2hip_synchronize(k2hip_model_t* model);

/* ---- OfflineStream (OfflineStream.cs:7-99): per-utterance feature buffer.
 * accept_samples = AddSamples (:43-57).  What a caller can observe is the reference's: speech_length counts the frames of
 * the streaming fbank over everything accepted so far (left-over samples shorter than a frame shift are carried to the
 * next call, as an OnlineFbank does; InputFinished is never called by the reference), get_speech returns them.
 * WHEN they are computed is not: the call only copies the samples into the stream's queue (no fbank launch, no lock on the
 * model); k2hip_offline_recognizer_get_results computes the whole batch's frames in one launch on the device, get_speech
 * computes this stream's.  The queue lives in PINNED host memory (~4 bytes per sample; the buffers of destroyed streams are
 * kept per model, at most 128 of them, and handed to the next streams), which the device reads in place. */
int32_t k2hip_offline_stream_create(k2hip_model_t* model, k2hip_offline_stream_t** out);
int32_t k2hip_offline_stream_destroy(k2hip_offline_stream_t* s);
int32_t k2hip_offline_stream_accept_samples(k2hip_offline_stream_t* s, const float* samples, int64_t n);
/* SpeechLength (float count) */
int64_t k2hip_offline_stream_speech_length(const k2hip_offline_stream_t* s);
/* copies Speech to out (cap floats) */
int32_t k2hip_offline_stream_get_speech(const k2hip_offline_stream_t* s, float* out, int64_t cap);
/* ---- token ids -> text (host only; no GPU involved) ------------------------------------------------------------------
 * OfflineRecognizer.DecodeMulti + CheckText + HexToStr (OfflineRecognizer.cs:432-565; online :321-352) and
 * Utils/ByteDataHelper.SmartByteDecode (:352-397): tokens.txt lookup (first space-separated field), stop at id 2, skip id -1
 * (offline), drop <blk> / <sos/eos> / <unk>, U+2581 -> ' ', <0x..> byte runs -> UTF-8, otherwise spaces removed + byte-BPE
 * decode, lower-case.  Text is UTF-8, NUL terminated; out == NULL only queries len (bytes without the NUL). */
int32_t k2hip_tokens_load(const char* tokens_path, k2hip_tokens_t** out);   /* File.ReadAllLines(tokensFilePath), :36 */
int32_t k2hip_tokens_destroy(k2hip_tokens_t* t);
int32_t k2hip_tokens_size(const k2hip_tokens_t* t);                          /* _tokens.Length (the CTC vocab_size, :325) */
int32_t k2hip_decode_text(const k2hip_tokens_t* t, const int64_t* ids, int32_t n, int32_t online, char* out, int32_t cap,
                          int32_t* len);
/* The byte-BPE alphabet the decode above uses: BYTE_TO_BCHAR[byte] as a code point (ByteDataHelper.cs:27-285,295-299;
 * -1 outside 0..255) and its inverse BCHAR_TO_BYTE (:300-304, BPE_UNK 8263 -> 32; -1 for a char outside the alphabet). */
int32_t k2hip_bbpe_char(int32_t byte);
int32_t k2hip_bbpe_byte(int32_t code_point);

/* ---- CTC models (Model_type "zipformer2ctc": OfflineProjOfZipformer2ctc / OnlineProjOfZipformer2ctc) -------------------
 * The encoder entry points (k2hip_offline_encoder, the online step) return log_probs [B,T',V] for such a model.
 * k2hip_ctc_greedy replaces the loop of ForwardBatchGreedySearchCTC (OfflineRecognizer.cs:383-408): y = first index of the
 * frame maximum (Array.IndexOf), emitted when y != blank and y != previous frame's y (prev_id = -1 at the start of every
 * call); timestamps get frame_offsets[b] added; num_trailing_blank[b] (in/out) follows :392-397.  The fused batch entries
 * (k2hip_offline_greedy*, get_results, k2hip_online_step) run this search automatically for a CTC model. */
int32_t k2hip_ctc_greedy(k2hip_model_t* model, const float* log_probs, int32_t B, int32_t Tprime, const int32_t* frame_offsets,
                         int64_t* tokens, int32_t* timestamps, int32_t* n_tokens, int32_t max_tokens, int32_t* num_trailing_blank);
/* OfflineStream.FrameOffset / NumTrailingBlank (OfflineStream.cs:39-40) */
int32_t k2hip_offline_stream_get_ctc_state(const k2hip_offline_stream_t* s, int32_t* frame_offset, int32_t* num_trailing_blank);

/* ---- decoding method --------------------------------------------------------------------------
 * The reference picks the search by the recognizer's `decodingMethod` string (OfflineRecognizer.cs:54-68) and only
 * knows "greedy_search".  BASELINE.json configs[2] adds "modified_beam_search" (icefall semantics, restated in
 * DESIGN.md): per stream at most `beam` hypotheses, log-softmax over the vocabulary, top-`beam` over
 * beam x V, equal token sequences merged by logaddexp, best hypothesis by length-normalised log-prob.
 * The setting is per model handle and applies to every BATCH entry point (k2hip_offline_greedy*,
 * k2hip_offline_recognizer_get_results, submit/wait) and to the streaming step (k2hip_online_step); the single-stream
 * offline path stays greedy, and a CTC model (zipformer2ctc) keeps its own CTC search under either setting.
 * "ctc_prefix_beam_search" (CTC models only; K2HIP_ERR_UNSUPPORTED for a transducer model): the batch entry points run the CTC prefix
 * beam search with beam `beam` ("CTC prefix beam search with N-best" below) and k2hip_last_scores returns the scores; the single-stream
 * path stays the collapse, and k2hip_online_step fails with K2HIP_ERR_INVALID while it is set (no stream changes).
 *
 * Streaming under modified_beam_search: after every k2hip_online_step a stream holds exactly what the offline search
 * (k2hip_beam_search, same tie-breaks) gives over ALL encoder frames the stream has produced so far -- its hypotheses live on
 * from one chunk to the next.  Start state: one hypothesis [blank, blank], log-prob 0.  Skip set {blank, unk} as offline
 * (not the greedy streaming rule {blank, unk, 1} of OnlineRecognizer.cs:181: the reference has no beam search, the project's
 * beam semantics hold).  Equal token sequences are merged on exact whole-sequence equality.  After each step:
 *   Tokens = [blank, blank] + the best hypothesis (highest log-prob / (length + 2), first in insertion order on ties),
 *   Hyp = its last two tokens, Timestamps = ABSOLUTE encoder frame indexes (frames of earlier chunks + t; the greedy path keeps
 *   the reference's chunk-relative ones), k2hip_online_stream_get_score = its log-prob.
 * The best hypothesis can revise earlier tokens: n_new_tokens is the SIGNED change of its length, and a host re-reads Tokens
 * after every step instead of appending.  A stream keeps the method and beam it decoded its first chunk with: after a change of
 * the setting, k2hip_online_step fails with K2HIP_ERR_INVALID for it until k2hip_online_stream_reset (which clears the
 * hypotheses).  With a hotword graph attached to the stream (k2hip_online_stream_set_hotwords, below) the same rule holds against
 * the BIASED offline search, and Tokens are revised from step to step more often (an unfinished match that led drops back): the
 * re-read contract above covers it. */
int32_t k2hip_set_decoding_method(k2hip_model_t* model, const char* method /* "greedy_search" | "modified_beam_search" | "ctc_prefix_beam_search" */,
                                  int32_t beam /* 1..8, ignored for greedy_search */);
/* operator level: modified beam search over a host encoder_out [B,T',J]; scores [B] (optional) = log-prob of the
 * returned hypothesis */
int32_t k2hip_beam_search(k2hip_model_t* model, const float* enc_out, int32_t B, int32_t Tprime, int32_t beam, int64_t* tokens,
                          int32_t* timestamps, int32_t* n_tokens, int32_t max_tokens, float* scores);
/* log-probs of the hypotheses returned by the last synchronous batch call made under modified_beam_search */
int32_t k2hip_last_scores(k2hip_model_t* model, float* scores, int32_t B);
/* operator level of the STREAMING beam search, for hosts that run their own encoder (csharp/OnlineProjOfHip.cs) and for tests:
 * a k2hip_beam_stream_t is one stream's hypotheses (host memory; no device slot).  k2hip_beam_search_chunk continues every
 * stream's search over Tc more frames of encoder_out [B, Tc, J] (any Tc >= 1, may vary between calls; all streams of a call
 * share one beam); afterwards a stream holds what k2hip_beam_search gives over all frames fed so far: tokens WITHOUT the
 * [blank, blank] prefix (as k2hip_beam_search), absolute timestamps, the log-prob of the best hypothesis.  A failed call
 * changes no stream.  The fused step (k2hip_online_step) runs the same kernel. */
int32_t k2hip_beam_stream_create(k2hip_model_t* model, int32_t beam /* 1..8 */, k2hip_beam_stream_t** out);
int32_t k2hip_beam_stream_destroy(k2hip_beam_stream_t* s);
int32_t k2hip_beam_stream_reset(k2hip_beam_stream_t* s);   /* back to the start state (an attached hotword graph stays) */
int32_t k2hip_beam_search_chunk(k2hip_model_t* model, k2hip_beam_stream_t* const* streams, int32_t B, const float* enc_out, int32_t Tc);
int32_t k2hip_beam_stream_num_tokens(const k2hip_beam_stream_t* s);
int32_t k2hip_beam_stream_get_tokens(const k2hip_beam_stream_t* s, int64_t* tokens, int32_t cap);
int32_t k2hip_beam_stream_get_timestamps(const k2hip_beam_stream_t* s, int32_t* timestamps, int32_t cap);
int32_t k2hip_beam_stream_get_score(const k2hip_beam_stream_t* s, float* score);

/* ---- hotword (contextual) biasing of the modified beam search, offline (per model) and streaming (per stream) ----------------
 * The reference never got this far (Utils/HotwordsHelper.cs is a helper without a call site: it has no beam search); the
 * semantics are the project's own, after icefall's ContextGraph, and are defined here and in DESIGN.md "Hotword biasing".
 *
 * Graph: P phrases, each a non-empty sequence of token ids in [0, vocab_size) without blank (0) and unk (2), and one
 * score_per_token c (finite, >= 0).  The trie of the phrases with Aho-Corasick failure links; state 0 is the root,
 * pending(s) = c * depth(s).  Creation fails with K2HIP_ERR_INVALID, the message naming the phrase, for: an empty phrase, an id
 * out of range, blank / unk inside a phrase, a phrase that is a proper prefix of another one, duplicate phrases, and a graph
 * over the size cap: the device form is dense (next state and bonus per (state, token)), so states * vocab_size may not exceed
 * K2HIP_HOTWORDS_MAX_ENTRIES.
 * Step: a hypothesis in state s that appends the real token v (blank and unk append nothing and leave s alone) moves to
 * n = delta(s, v) (goto; on a miss the failure links; the root loops on a miss) and its log-prob gets pending(n) - pending(s)
 * (negative when a partial match breaks).  If n ends a phrase the match is committed: the bonus stays, the new state is the root.
 * A phrase end reachable only through a failure link from n is NOT reported (no output links) -- limitation of this version.
 * Search: a frame's top-`beam` selection uses the unbiased sums as before; the bonus of a selected candidate is added before the
 * candidates that spell the same sequence are merged (logaddexp of the biased scores; the merged hypothesis keeps the
 * first-inserted one's state).  After the last frame every hypothesis loses pending(state) (an unfinished match earns nothing),
 * then the usual length-normalised pick; scores report the finalized log-prob.
 * A k2hip_hotwords_t belongs to no model and needs no GPU. */
#define K2HIP_HOTWORDS_MAX_ENTRIES (1 << 23)
/* ids: the phrases' tokens back to back, lens [n_phrases] */
int32_t k2hip_hotwords_create(const int64_t* ids, const int32_t* lens, int32_t n_phrases, float score_per_token, int32_t vocab_size,
                              k2hip_hotwords_t** out);
/* a text file, one phrase per line, written as the token strings of tokens.txt separated by blanks ("▁HE LL O"; the
 * pre-tokenised form -- no BPE encoder here); lines without a token are skipped; an unknown token string fails with the line
 * number, and so does everything k2hip_hotwords_create refuses (vocab_size = the number of lines of tokens.txt) */
int32_t k2hip_hotwords_load(const k2hip_tokens_t* tokens, const char* path, float score_per_token, k2hip_hotwords_t** out);
int32_t k2hip_hotwords_destroy(k2hip_hotwords_t* hw);
int32_t k2hip_hotwords_num_states(const k2hip_hotwords_t* hw);   /* -1 for NULL */
/* the host walk of the definition above (for tests and for hosts that score a transcript) */
int32_t k2hip_hotwords_step(const k2hip_hotwords_t* hw, int32_t state, int64_t token, int32_t* next_state, float* bonus);
int32_t k2hip_hotwords_pending(const k2hip_hotwords_t* hw, int32_t state, float* pending);
/* hw = NULL clears.  Checks vocab_size against the model, uploads the tables (the model keeps its own copy: hw may be destroyed
 * afterwards) and keeps them until replaced or the model is destroyed; not while submitted batches are in flight.  Applies wherever
 * the offline modified beam search runs: k2hip_beam_search and the batch entry points under
 * k2hip_set_decoding_method("modified_beam_search") (k2hip_offline_greedy*, k2hip_offline_recognizer_get_results, submit / wait).
 * Greedy search, the CTC search and the single-stream path ignore it (the CTC prefix beam search uses it once
 * k2hip_set_ctc_prefix_biasing is on).  No hotwords, or an empty list: bit for bit the unbiased
 * results.  This list is the OFFLINE batch's: with it set, k2hip_beam_search_chunk and k2hip_online_step under
 * modified_beam_search fail with K2HIP_ERR_INVALID, graphs attached to the streams or not (streaming greedy is untouched).
 * STREAMING takes its graph per stream, below. */
int32_t k2hip_set_hotwords(k2hip_model_t* model, const k2hip_hotwords_t* hw);
/* STREAMING: the graph belongs to the stream (each connection brings its own list).  hw = NULL detaches.  Checks vocab_size against
 * the stream's model; the stream keeps its own reference to the uploaded tables, so hw may be destroyed afterwards.  Streams that
 * attach the same k2hip_hotwords_t to the same model share one upload; the tables are freed when the last such stream is detached
 * or destroyed, or with the model (a stream may be destroyed before or after its model as far as the graph is concerned).
 * Allowed only while the stream holds the start state -- before its first decoded chunk or after k2hip_online_stream_reset /
 * k2hip_beam_stream_reset -- else K2HIP_ERR_INVALID ("... reset the stream first"): saved hypotheses carry states of the graph they
 * started with.  A reset keeps the graph and returns every hypothesis to the root.
 * Semantics: after every step (k2hip_online_step under modified_beam_search, k2hip_beam_search_chunk) the stream holds exactly
 * what the offline biased search (k2hip_beam_search with the same graph set by k2hip_set_hotwords) gives over ALL encoder frames
 * produced so far.  Every saved hypothesis carries its graph state across the chunk boundary, and its carried log-prob KEEPS the
 * pending bonus (the match may complete in the next chunk).  Per step the best hypothesis is picked on
 * (log-prob - pending(state)) / (length + 2), first maximum, and k2hip_online_stream_get_score / k2hip_beam_stream_get_score
 * report log-prob - pending(state) of that pick; nothing is subtracted from what is carried.  Tokens can therefore be revised from
 * step to step more often than without a graph: re-read them after every step (n_new_tokens is a signed change).
 * One call may mix streams with different graphs and streams with none; a call in which no stream has a graph is exactly the
 * unbiased call.  An empty graph or score_per_token = 0: bit for bit the unbiased results.  Streaming greedy search and a CTC model's
 * search ignore an attached graph -- unless the CTC stream opts in with k2hip_online_stream_set_ctc_prefix_biasing (below, "Biasing of
 * the streaming CTC prefix beam search"). */
int32_t k2hip_online_stream_set_hotwords(k2hip_online_stream_t* s, const k2hip_hotwords_t* hw);
int32_t k2hip_beam_stream_set_hotwords(k2hip_beam_stream_t* s, const k2hip_hotwords_t* hw);

/* ---- n-gram LM shallow fusion in the modified beam search, offline and streaming ----------------------------------------------------------------
 * The reference has no beam search and no LM; the semantics are the project's own, defined here and in DESIGN.md "N-gram LM
 * shallow fusion".
 *
 * LM: a back-off n-gram of order N, 1 <= N <= 5, over the model's own token ids.  An entry is (ids[1..n], log_prob, backoff), natural
 * log, float32, backoff 0 where absent.  Blank (0) and unk (2) may not occur in an entry; the sentence marks and the LM's own unknown
 * word are the pseudo ids below.  Automaton: state 0 is the empty history; one state per history of length 1 .. N-1 that is the
 * history of some kept entry, numbered by (length, then ids lexicographically, <s> = -1 first).  A state has its explicit arcs
 * (token -> log_prob, next state), a back-off weight (the backoff of the history's own entry) and a back-off state (the longest
 * proper suffix of its history that is a state).  The next state of (h, w) is the longest suffix of h.w, of length <= N-1, that is
 * a state.
 * Step(s, w), w a real token: acc = 0; while w has no arc in s and s != 0: acc = acc + bow(s), s = backoff(s); the result is
 * acc + log_prob(arc), in float32 in exactly that order.  At state 0 a token without a unigram scores the LM's <unk> unigram and
 * moves to state 0; if such a token exists and the LM has no <unk> unigram, creation fails and names the first such token.  Blank and
 * unk append nothing: state unchanged, 0.
 * Start state: the state of history <s> if the LM has kept entries with that history, else 0.  </s> and <s> as PREDICTED words are
 * ignored (the <s> unigram still gives the back-off weight of history <s>); n-grams of order >= 2 that contain <unk> are dropped (a
 * token without a unigram returns to state 0, so they are never reached).  No end-of-sentence cost is ever applied.
 * Creation fails with K2HIP_ERR_INVALID, naming the entry (or the line), for: an order outside [1, 5], an id out of range, blank / unk
 * in an entry, a sentence mark inside a history, a non-finite number, a duplicate entry, an n-gram whose history has no entry of its
 * own, and a model of more than K2HIP_NGRAM_MAX_ARCS entries.
 * A k2hip_ngram_lm_t belongs to no model and needs no GPU. */
#define K2HIP_NGRAM_MAX_ARCS (1 << 24)
#define K2HIP_NGRAM_MAX_ORDER 5
#define K2HIP_NGRAM_BOS (-1) /* <s> */
#define K2HIP_NGRAM_EOS (-2) /* </s> */
#define K2HIP_NGRAM_UNK (-3) /* the LM's <unk>: the fallback for tokens without a unigram, never the acoustic unk id */
/* ids: the entries' tokens back to back; orders / log_probs / backoffs [n_entries] */
int32_t k2hip_ngram_lm_create(const int64_t* ids, const int32_t* orders, const float* log_probs, const float* backoffs, int64_t n_entries,
                              int32_t vocab_size, k2hip_ngram_lm_t** out);
/* a text ARPA file whose words are the token strings of tokens.txt.  <unk> is always the LM's fallback; <s> and </s> are the
 * sentence marks unless they are themselves lines of tokens.txt.  log10 values are parsed as double, multiplied by ln 10 in double,
 * then rounded to float32.  Refused with K2HIP_ERR_INVALID and the line number: a missing \data\ or \end\, counts that disagree with
 * the sections, an order above 5, an unknown word, a non-finite number, and everything k2hip_ngram_lm_create refuses. */
int32_t k2hip_ngram_lm_load(const k2hip_tokens_t* tokens, const char* path, k2hip_ngram_lm_t** out);
int32_t k2hip_ngram_lm_destroy(k2hip_ngram_lm_t* lm);
int32_t k2hip_ngram_lm_order(const k2hip_ngram_lm_t* lm);        /* -1 for NULL, as the next three */
int32_t k2hip_ngram_lm_num_states(const k2hip_ngram_lm_t* lm);
int64_t k2hip_ngram_lm_num_arcs(const k2hip_ngram_lm_t* lm);
int32_t k2hip_ngram_lm_start_state(const k2hip_ngram_lm_t* lm);
/* the host walk of Step above, unscaled */
int32_t k2hip_ngram_lm_step(const k2hip_ngram_lm_t* lm, int32_t state, int64_t token, int32_t* next_state, float* log_prob);
/* lm = NULL clears; scale finite and >= 0.  Checks vocab_size against the model and uploads the sparse tables, every weight
 * multiplied by scale once on the host in float32 (the device only adds); the model keeps its own copy, so lm may be destroyed
 * afterwards.  Not while submitted batches are in flight.
 * Search: every hypothesis carries an LM state, the start hypothesis the start state.  A frame's top-`beam` selection uses the same
 * sums as without an LM; a selected candidate that appends a real token v then gets (sum + hotword bonus) + Step(state, v), and
 * the merge of candidates that spell the same sequence follows.  Blank and unk leave the state alone and earn nothing.  Nothing is
 * pending or taken back at the end: the final pick and every reported score (N-best scores included) use the log-prob with the LM
 * terms.  Token log-probs and the beam trace stay the unbiased acoustic terms.  Works together with k2hip_set_hotwords and
 * k2hip_set_nbest.
 * One setting per model.  Unlike the model-level hotword list it applies to BOTH searches: wherever the offline modified beam search
 * runs (as k2hip_set_hotwords), and in the streaming one (k2hip_online_step under modified_beam_search, k2hip_beam_search_chunk),
 * together with the streams' own hotword graphs.  Greedy search, the CTC search and the single-stream path ignore it (the CTC prefix
 * beam search uses it once k2hip_set_ctc_prefix_biasing is on).  No LM, a
 * cleared LM and scale = 0: bit for bit the plain results, from the plain kernels.
 * STREAMING: after every step a stream holds exactly what the offline search with the same LM gives over all frames so far; the LM
 * state of every saved hypothesis crosses the chunk boundary.  A stream keeps the LM setting it decoded its first chunk with: after
 * k2hip_set_ngram_lm changes or clears it (every call that leaves an LM set is a new setting; scale = 0 is "none"), k2hip_online_step
 * and k2hip_beam_search_chunk fail with K2HIP_ERR_INVALID ("... reset the stream first") for a call that names such a stream, and the
 * failed call changes no stream.  A reset returns every hypothesis to the start state of the LM then set.  A k2hip_set_ngram_lm that
 * lands between a streaming call's checks and its launch is caught under the lock that covers the launch (K2HIP_ERR_INVALID,
 * "... call again"; no stream changes): saved LM states never meet another LM's tables. */
int32_t k2hip_set_ngram_lm(k2hip_model_t* model, const k2hip_ngram_lm_t* lm, float scale);

/* ---- N-best hypotheses and token log-probs of the modified beam search ---------------------------------------------------------
 * Token log-prob: when a selected candidate (hypothesis k, token v), v outside {blank, unk}, is appended at frame t, its token
 * log-prob is the float32 term (logit[k][v] - max_k) - lse_k the step forms before it adds the hypothesis' log-prob -- that term
 * itself, not a difference of scores.  It is UNBIASED (a hotword bonus is never part of it) and <= 0.  It travels with the
 * timestamp: when candidates that spell the same sequence merge, the first-inserted hypothesis keeps its token log-probs exactly as
 * it keeps its timestamps.
 * N-best: after the last frame the surviving hypotheses (at most `beam`, pairwise distinct sequences) are ordered by the quantity of
 * the final pick, (log-prob - pending(state)) / (length + 2) (pending only with hotwords attached), descending, ties in insertion
 * order.  Entry 0 is therefore the result the search returns anyway: same tokens, timestamps and score.  Every entry carries its
 * tokens (no [blank, blank] prefix), timestamps, token log-probs and its FINALIZED log-prob (not the normalised value).  nbest is
 * in 1..8; asking for more than survive returns what survives.
 * Streaming: after every step a stream's alternatives are what the offline search gives over all frames so far (the contract of the
 * best result); they may be revised from step to step.  Their scores use the pending table attached when they are read.
 * What a stream holds before its first result, after a reset and after a failed call (offline streams: a failed GetResults; the
 * streaming calls change no stream when they fail) is the start state: ONE empty alternative with score 0.
 *
 * k2hip_set_nbest(model, n): n = 1 (the default) is off -- nothing is computed or kept beyond the best hypothesis.  With n > 1 the
 * synchronous entries k2hip_offline_recognizer_get_results, k2hip_online_step and k2hip_beam_search_chunk keep up to n alternatives
 * per stream, each with its token log-probs (token log-probs are recorded for the frames searched while n > 1; 0 for frames
 * searched before).  Needs modified_beam_search (K2HIP_ERR_INVALID under greedy_search, K2HIP_ERR_UNSUPPORTED for a CTC model), and
 * no submitted batch in flight.  A CTC model has alternatives under ctc_prefix_beam_search only (n <= its beam; UNSUPPORTED under its
 * other two methods): k2hip_offline_recognizer_get_results then fills the offline streams' alternatives, and leaving that method sets n
 * back to 1.  While n > 1: the pipelined k2hip_offline_submit_* / k2hip_offline_wait return K2HIP_ERR_INVALID (they
 * have one result per stream), and so does k2hip_offline_recognizer_get_result (the single-stream path is greedy search). */
int32_t k2hip_set_nbest(k2hip_model_t* model, int32_t n /* 1..8 */);
/* operator level: k2hip_beam_search that returns the list.  tokens / timestamps / token_log_probs [B][nbest][max_tokens],
 * n_tokens / scores [B][nbest], n_hyps [B] = entries written for the stream (<= min(beam, nbest)); what lies behind them is not
 * touched.  K2HIP_ERR_CAPACITY if any returned entry is longer than max_tokens -- also where the best one alone would fit: the
 * overflow rule of the single result holds per entry, and one over-long entry fails the whole call (the same holds for the
 * synchronous entries under k2hip_set_nbest(n > 1)).  Independent of k2hip_set_nbest. */
int32_t k2hip_beam_search_nbest(k2hip_model_t* model, const float* enc_out, int32_t B, int32_t Tprime, int32_t beam, int32_t nbest,
                                int64_t* tokens, int32_t* timestamps, float* token_log_probs, int32_t* n_tokens, int32_t* n_hyps,
                                float* scores, int32_t max_tokens);
/* ---- Forced alignment and full-sum scoring of a given transcript on the RNN-T lattice ------------------------------------------
 * No reference counterpart: the reference only searches.  The semantics are the project's own, defined here and in DESIGN.md "Forced
 * alignment and full-sum scoring"; they follow the modified beam search, so the scores are comparable with k2hip_beam_search when
 * no hotwords and no LM are set.
 * Per stream: frames t = 0 .. T-1; the target y_1 .. y_U, ids in [0, V), neither blank (0) nor unk (2).  The context of position u
 * is the last context_size ids of [blank, blank, y_1 .. y_u] (the offline beam search's start state), and
 * lp(t,u,.) = log_softmax(output_linear(tanh(enc[t] + decoder(ctx_u)))).  Arcs (modified topology, at most one symbol per frame):
 *   stay(t,u) = logaddexp(lp(t,u,blank), lp(t,u,unk)): (t,u) -> (t+1,u)   (the search's skip set is {blank, unk}, and two candidates
 *                                                                         that append nothing spell the same sequence and merge)
 *   emit(t,u) = lp(t,u,y_{u+1}):                       (t,u) -> (t+1,u+1), u < U
 * total_logp = logsumexp over all paths (0,0) -> (T,U) = log P(transcript | audio); best_logp = their maximum (Viterbi);
 * timestamps[u] = the frame t of the best path's emit arc of y_{u+1} (the search's convention; strictly increasing);
 * token_log_probs[u] = that arc's emit value (<= 0, as with k2hip_*_get_token_log_probs).
 * Tie rule of the Viterbi step: on equal float32 values the emit predecessor (t-1,u-1) wins over the stay predecessor (t-1,u).
 * All arithmetic is float32; logaddexp(a,b) = m + log1p(exp(min - m)), -inf operands give no NaN.
 * Hotwords and the n-gram LM set on the model are IGNORED: the lattice scores the acoustic model alone.  The model's decoding
 * method, N-best setting and later searches are not affected.
 * Errors: U > T has no path: K2HIP_ERR_INVALID, checked on the host before any device work, the message names the stream; so are a
 * blank, unk or out-of-vocabulary target id and n_frames outside [1, Tprime].  A CTC model: K2HIP_ERR_UNSUPPORTED.  U = 0 is legal:
 * total = best = the sum of stay(t,0).  K2HIP_ERR_CAPACITY if any lens[b] > max_tokens; nothing is written then.
 *
 * k2hip_transducer_align: operator level, enc_out [B][Tprime][joiner_dim] on the host.  n_frames [B] or NULL (= Tprime for every
 * stream); ids: the B targets back to back; lens [B].  Outputs, each may be NULL: timestamps / token_log_probs [B][max_tokens] (the
 * first lens[b] entries of row b are written), total_logp / best_logp [B].
 * k2hip_offline_align_from_samples: samples -> fbank -> pad -> encoder as k2hip_offline_greedy_from_samples, encoder_out stays on
 * the device; every stream is aligned over ALL Tprime frames of the padded batch, exactly the frames the searches decode.
 * *Tprime_out (may be NULL) = that frame count. */
int32_t k2hip_transducer_align(k2hip_model_t* model, const float* enc_out, int32_t B, int32_t Tprime, const int32_t* n_frames,
                               const int64_t* ids, const int32_t* lens, int32_t* timestamps, float* token_log_probs, float* total_logp,
                               float* best_logp, int32_t max_tokens);
int32_t k2hip_offline_align_from_samples(k2hip_model_t* model, const float* const* samples, const int64_t* n_samples, int32_t B,
                                         const int64_t* ids, const int32_t* lens, int32_t* timestamps, float* token_log_probs,
                                         float* total_logp, float* best_logp, int32_t max_tokens, int32_t* Tprime_out);
/* ---- Keyword spotting for transducer models: trie Viterbi on the lattice ---------------------------------------------------------
 * No reference counterpart (its Utils/HotwordsHelper.cs has no call site): the semantics are the project's own, defined here and in
 * DESIGN.md "Keyword spotting"; tests/kws_twin.py restates them in float64.
 *
 * Graph (k2hip_keywords_t): host only, needs no GPU and belongs to no model.  P >= 0 keywords, each a non-empty sequence of token ids
 * in [0, vocab_size) without blank (0) and unk (2) (id 1 is allowed), each with a threshold in (0, 1].  Creation fails with
 * K2HIP_ERR_INVALID, the message naming the keyword, for: an empty keyword, an id out of range, blank or unk inside a keyword, a
 * duplicate, a threshold outside (0, 1] or not finite, more than K2HIP_KEYWORDS_MAX_STATES trie states.  A keyword may be a proper
 * prefix of another: a terminal state may have children.  Trie states are numbered in insertion order, root = 0, parent(s) < s; state
 * s has tok(s), depth(s), kw(s) = the keyword ending there or -1, and bar(s) = (float)depth(s) * logf(threshold): one float32 product,
 * rounded once, on the host.  ctx(s) = the last context_size ids of [blank] * context_size + path(s).
 *
 * Arcs (the modified topology, at most one symbol per frame, exactly as in "Forced alignment and full-sum scoring"):
 *   lp(t,s,.) = log_softmax(output_linear(tanh(enc[t] + decoder(ctx(s)))))
 *   stay(t,s) = logaddexp(lp(t,s,blank), lp(t,s,unk));  for c != root: emit(t,c) = lp(t, parent(c), tok(c)).
 *
 * Token passing, per stream, all in float32.  Frames are numbered absolutely, t = 0, 1, .., since the stream's creation or reset.
 * Every non-root state holds (a, start), initially a = -inf; the root always holds (0, t): a keyword may begin at any frame at no
 * cost.  For every non-root c, from the values before frame t:
 *   ve = a[parent(c)] + emit(t,c)   (a root parent contributes 0 and start = t),   vs = a[c] + stay(t,c),   a[c] <- max(ve, vs);
 * the emit predecessor wins an exact float32 tie, `start` is inherited from the winner, and if both are -inf the state stays -inf.
 *
 * Detection, after the update of frame t: among the terminal states that were entered by their emit arc in this frame and have
 * a[c] >= bar(c) (the average log-prob per keyword token reaches log threshold) the winner is the one of largest depth, then largest
 * a, then smallest keyword index.  At most one event fires per frame: (keyword, start, end = t, sum_logp = a[c]).  After it every
 * non-root state is set to -inf (overlapping matches are suppressed); the root restarts at t + 1.  The device compares and adds only;
 * score = sum_logp / depth is computed by the host accessors.
 *
 * Streaming rule: after any chunking a stream's events and carried (a, start) are bit for bit those of one call over all frames so
 * far.  n_frames[b] = 0 leaves stream b untouched.  Zero keywords (one state) is legal and never fires.
 * Hotwords, the n-gram LM and the decoding method do not take part.  A CTC model: K2HIP_ERR_UNSUPPORTED (its spotter is
 * k2hip_ctc_kws_* / k2hip_offline_ctc_spot_keywords_from_samples, "Keyword spotting for CTC models" below).  Every transducer family is
 * served: the search consumes encoder_out [B][T][joiner_dim] only.
 *
 * k2hip_keywords_create: keyword p = ids[off .. off + lens[p]), thresholds[p].  k2hip_keywords_load: a text file in the token-string
 * form of k2hip_hotwords_load, one keyword per line (empty lines are skipped); an optional last field ":0.35" gives the line's threshold,
 * default_threshold the others'; errors name the line.
 * k2hip_kws_stream_create: a stream of `kw` on `model` (K2HIP_ERR_INVALID if the graph's vocab_size is not the model's).  The graph's
 * decoder rows are computed once per (model, graph), kept on the device and shared by the streams of that pair; the stream keeps its own
 * reference to the graph, so `kw` may be destroyed at once.  k2hip_kws_stream_reset: frame count 0, no tokens, no events.
 * k2hip_kws_search_chunk: enc_out [B][Tc][joiner_dim] on the host, any Tc >= 1, n_frames [B] in [0, Tc] or NULL (= Tc); the streams
 * (distinct, all of `model`) may walk different graphs.  New events are appended to each stream's list.  A failed call changes no
 * stream.
 * k2hip_kws_stream_get_events: the first min(cap, n) events into the arrays (each may be NULL), returns their number n or an error;
 * score[i] = sum_logp[i] / (number of tokens of keyword[i]).
 * k2hip_offline_spot_keywords_from_samples: samples -> fbank -> pad -> encoder as k2hip_offline_greedy_from_samples, encoder_out stays
 * on the device; fresh streams of `kw`, every one searched over ALL Tprime frames of the padded batch.  Outputs [B][max_events] (each
 * may be NULL), n_events [B]; K2HIP_ERR_CAPACITY if a stream has more events than max_events.  *Tprime_out (may be NULL) = the frame
 * count. */
#define K2HIP_KEYWORDS_MAX_STATES 1024
int32_t k2hip_keywords_create(const int64_t* ids, const int32_t* lens, const float* thresholds, int32_t n_keywords, int32_t vocab_size,
                              k2hip_keywords_t** out);
int32_t k2hip_keywords_load(const k2hip_tokens_t* tokens, const char* path, float default_threshold, k2hip_keywords_t** out);
int32_t k2hip_keywords_destroy(k2hip_keywords_t* kw);
int32_t k2hip_keywords_num_states(const k2hip_keywords_t* kw);
int32_t k2hip_keywords_num_keywords(const k2hip_keywords_t* kw);
int32_t k2hip_kws_stream_create(k2hip_model_t* model, const k2hip_keywords_t* kw, k2hip_kws_stream_t** out);
int32_t k2hip_kws_stream_destroy(k2hip_kws_stream_t* s);
int32_t k2hip_kws_stream_reset(k2hip_kws_stream_t* s);
int64_t k2hip_kws_stream_num_frames(const k2hip_kws_stream_t* s);
int32_t k2hip_kws_search_chunk(k2hip_model_t* model, k2hip_kws_stream_t* const* streams, int32_t B, const float* enc_out, int32_t Tc,
                               const int32_t* n_frames);
int32_t k2hip_kws_stream_num_events(const k2hip_kws_stream_t* s);
int32_t k2hip_kws_stream_get_events(const k2hip_kws_stream_t* s, int32_t* keyword, int32_t* start, int32_t* end, float* sum_logp, float* score,
                                    int32_t cap);
int32_t k2hip_kws_stream_clear_events(k2hip_kws_stream_t* s);
int32_t k2hip_offline_spot_keywords_from_samples(k2hip_model_t* model, const k2hip_keywords_t* kw, const float* const* samples,
                                                 const int64_t* n_samples, int32_t B, int32_t* keyword, int32_t* start, int32_t* end,
                                                 float* sum_logp, float* score, int32_t* n_events, int32_t max_events, int32_t* Tprime_out);
/* ---- Keyword spotting for CTC models: trie Viterbi on the CTC trellis (zipformer2ctc models) -------------------------------------
 * No reference counterpart: the semantics are the project's own, defined here and in DESIGN.md "CTC keyword spotting"; they follow
 * "Keyword spotting" and "CTC forced alignment" wherever those already decide a question.  tests/ctc_kws_twin.py restates them in
 * float64, csrc/ctc_kws_ref.h in float32.
 *
 * Graph: a k2hip_keywords_t as it is, with all its refusals.  Limitation: it keeps refusing unk (id 2) inside a keyword although CTC
 * treats unk as an ordinary token.  bar(s) = (float)depth(s) * logf(threshold) as before.  One derived host table: rc(s) = the root's
 * child whose token equals tok(s), or -1.
 *
 * Input: lp(t, v), a row's log-probs [T][V], finite or -inf; blank is id 0.
 *
 * States: every non-root trie state c holds two cells, n[c] (the path's last frame carried tok(c)) and b[c] (tok(c) is finished and
 * the path sits in blanks after it).  Each cell is (value, start), initially (-inf, -1).  The root is free: value 0, start t -- a
 * keyword may begin at any frame at no cost.
 *
 * Frame t: all reads are of the values before the frame; all arithmetic is float32, adds and compares only.
 *   n[c] <- max(pred, n[c]) + lp(t, tok(c)).  When parent(c) is the root, pred is the root (0, t).  Otherwise pred is the better of
 *     n[parent(c)] and b[parent(c)], n[parent(c)] being allowed only when tok(parent(c)) != tok(c): a repeated token needs a blank
 *     between, the CTC rule.  Exact float32 ties go in k2hip_ctc_align's order (lowest extended-state index first): n[parent], then
 *     b[parent], then the self loop.  c is "entered" in this frame when the winner is not the self loop and the result is above -inf.
 *   b[c] <- max(n[c], b[c]) + lp(t, 0); on a tie n[c] wins.
 *   `start` is inherited from the winner; a cell at -inf carries start = -1.
 *
 * Hold, the one rule CTC needs beyond the transducer spotter: a CTC token may span several frames, so a keyword whose tokens are all
 * the same -- in practice a one-token keyword -- would fire again on each of them.  Each stream carries `hold`, a state index or -1.
 * At the top of frame t, if hold = r >= 0: when lp(t, tok(r)) >= lp(t, 0) the root arc into r is closed for this frame; otherwise
 * hold <- -1 and the arc is open.  An event whose winner is c sets hold <- rc(c), effective from frame t + 1.
 *
 * Detection, after the update of frame t: among the terminal states entered in this frame with n[c] >= bar(c) the winner is the one of
 * largest depth, then largest n[c], then smallest keyword index.  At most one event fires per frame: (keyword, start, end = t,
 * sum_logp = n[c]).  After an event every non-root cell becomes (-inf, -1).  score = sum_logp / depth is computed by the host
 * accessors.
 *
 * Carried block (canonical: one function of the frames seen, whatever the chunking): values [2][S] floats and starts [2][S] ints,
 * plane 0 = n, plane 1 = b.  The root's n entry is (0, frame count); the root's b entry is (-inf, hold).
 *
 * Streaming rule: after any chunking a stream's events and carried block are bit for bit those of one call over all frames so far.
 * n_frames[b] = 0 leaves stream b untouched.  Zero keywords is legal and never fires.  Streams in one call may walk different graphs.
 * A failed call changes no stream.
 *
 * The entries follow the argument rules of their k2hip_kws_* siblings.  k2hip_ctc_kws_search_chunk: log_probs [B][Tc][V] on the host
 * (as k2hip_online_encoder returns them for a streaming CTC model), any Tc >= 1, n_frames [B] in [0, Tc] or NULL (= Tc).  A stream
 * keeps its own reference to the graph, so `kw` may be destroyed at once; the graph's tables are uploaded with every call (there are
 * no decoder rows to keep resident).  k2hip_offline_ctc_spot_keywords_from_samples: samples -> fbank -> pad -> encoder, the log-probs
 * stay on the device; fresh streams of `kw`, every one searched over ALL Tprime frames of the padded batch; K2HIP_ERR_CAPACITY if a
 * stream has more events than max_events.
 * Refusals, all decided on the host before any device work: K2HIP_ERR_UNSUPPORTED for a transducer model; K2HIP_ERR_INVALID for a
 * graph of another vocabulary size, a stream listed twice, a stream of another model, n_frames[b] outside [0, Tc]. */
int32_t k2hip_ctc_kws_stream_create(k2hip_model_t* model, const k2hip_keywords_t* kw, k2hip_ctc_kws_stream_t** out);
int32_t k2hip_ctc_kws_stream_destroy(k2hip_ctc_kws_stream_t* s);
int32_t k2hip_ctc_kws_stream_reset(k2hip_ctc_kws_stream_t* s);
int64_t k2hip_ctc_kws_stream_num_frames(const k2hip_ctc_kws_stream_t* s);
int32_t k2hip_ctc_kws_search_chunk(k2hip_model_t* model, k2hip_ctc_kws_stream_t* const* streams, int32_t B, const float* log_probs, int32_t Tc,
                                   const int32_t* n_frames);
int32_t k2hip_ctc_kws_stream_num_events(const k2hip_ctc_kws_stream_t* s);
int32_t k2hip_ctc_kws_stream_get_events(const k2hip_ctc_kws_stream_t* s, int32_t* keyword, int32_t* start, int32_t* end, float* sum_logp,
                                        float* score, int32_t cap);
int32_t k2hip_ctc_kws_stream_clear_events(k2hip_ctc_kws_stream_t* s);
int32_t k2hip_offline_ctc_spot_keywords_from_samples(k2hip_model_t* model, const k2hip_keywords_t* kw, const float* const* samples,
                                                     const int64_t* n_samples, int32_t B, int32_t* keyword, int32_t* start, int32_t* end,
                                                     float* sum_logp, float* score, int32_t* n_events, int32_t max_events, int32_t* Tprime_out);
/* ---- CTC forced alignment and full-sum scoring of given transcripts (zipformer2ctc models) -------------------------------------
 * No reference counterpart: the reference's CTC path only searches (ForwardBatchGreedySearchCTC).  The semantics are the project's
 * own, defined here and in DESIGN.md "CTC forced alignment and full-sum scoring".
 * log_probs [R][Tprime][V] is what the encoder entries of a CTC model return, already log-softmaxed; lp(t, v) is row r's entry.  A
 * target y_1 .. y_U is scored against row r over that row's first T = n_frames[r] frames.
 * Target ids lie in [1, V): only blank (0) is illegal; unk is legal, because the CTC search does not filter it either.
 * Topology (standard CTC): the extended sequence z = [blank, y_1, blank, y_2, .., y_U, blank] with S = 2U + 1 states.  State s at
 * frame t is reached from s, from s-1, and from s-2; the s-2 predecessor is allowed only when z_s is not blank and z_s != z_{s-2}.
 * Every arrival pays lp(t, z_s).  Frame 0 starts in state 0 or state 1.  The path ends after frame T-1 in state S-1 or S-2.
 * total_logp = the log-sum-exp over all such paths = log P(transcript | audio); best_logp = their maximum (Viterbi);
 * timestamps[u] = the first frame the best path spends in y_{u+1}'s state (the frame at which the CTC greedy collapse would emit the
 * token); end_frames[u] = the last frame it spends there (timestamps[u] <= end_frames[u] < timestamps[u+1]);
 * token_log_probs[u] = lp(timestamps[u], y_{u+1}).
 * All arithmetic is float32; logaddexp(a,b) = m + log1p(exp(min - m)), -inf operands give no NaN.  If every path crosses a -inf
 * cell, best_logp = total_logp = -inf and the three per-token outputs are unspecified (inside [0, T) and finite or -inf).
 * Tie rule of the Viterbi step: on equal float32 values the predecessor with the lowest state index wins -- s-2 over s-1 over s; at
 * the end S-2 wins over S-1.
 * U = 0 is legal: total = best = the sum of lp(t, blank).  A target needs T >= U + (the number of adjacent equal pairs in y), else it
 * has no path: K2HIP_ERR_INVALID, decided on the host before any device work, the message names the target ("target h"); so are a
 * blank or out-of-range id, n_frames outside [1, Tprime] and a stream_of entry outside [0, R).  At most 4095 tokens per target and
 * 65535 targets per call (K2HIP_ERR_INVALID beyond).  K2HIP_ERR_CAPACITY if any lens[h] > max_tokens; nothing is written then.  A
 * transducer model has no CTC head: K2HIP_ERR_UNSUPPORTED.  (k2hip_transducer_align / k2hip_offline_align_from_samples keep refusing a
 * CTC model.)
 *
 * k2hip_ctc_align: operator level, log_probs [R][Tprime][V] on the host.  n_frames [R] or NULL (= Tprime for every row).  H targets:
 * ids = the targets back to back, lens [H]; stream_of [H] names the row each target is scored against, NULL = H == R and the identity
 * (rescoring a candidate list against one utterance is one call with no duplicated activations).  Outputs, each may be NULL:
 * timestamps / end_frames / token_log_probs [H][max_tokens] (the first lens[h] entries of row h are written), total_logp / best_logp [H].
 * k2hip_offline_ctc_align_from_samples: samples -> fbank -> pad -> encoder as k2hip_offline_greedy_from_samples, log_probs stay on
 * the device (R = B); every target is aligned over ALL Tprime frames of the padded batch, exactly the frames the CTC search decodes.
 * *Tprime_out (may be NULL) = that frame count. */
int32_t k2hip_ctc_align(k2hip_model_t* model, const float* log_probs, int32_t R, int32_t Tprime, const int32_t* n_frames, int32_t H,
                        const int32_t* stream_of, const int64_t* ids, const int32_t* lens, int32_t* timestamps, int32_t* end_frames,
                        float* token_log_probs, float* total_logp, float* best_logp, int32_t max_tokens);
int32_t k2hip_offline_ctc_align_from_samples(k2hip_model_t* model, const float* const* samples, const int64_t* n_samples, int32_t B, int32_t H,
                                             const int32_t* stream_of, const int64_t* ids, const int32_t* lens, int32_t* timestamps,
                                             int32_t* end_frames, float* token_log_probs, float* total_logp, float* best_logp,
                                             int32_t max_tokens, int32_t* Tprime_out);
/* ---- CTC prefix beam search with N-best (zipformer2ctc models) -------------------------------------------------------------------
 * No reference counterpart: the reference's CTC path only does ForwardBatchGreedySearchCTC.  The semantics are the project's own,
 * defined here, in DESIGN.md "CTC prefix beam search" and, as code, in csrc/ctc_prefix_ref.h.
 * log_probs [R][Tprime][V] is what the encoder entries of a CTC model return; lp(t, v) is row r's entry.  Row r is searched over its
 * first T = n_frames[r] frames (NULL = Tprime).  Blank is id 0; every other id, unk included, is an ordinary token, as in the CTC
 * collapse and k2hip_ctc_align.
 * A live hypothesis is a prefix y (a token sequence) with two float32 log-probs: pb (paths ending in blank) and pnb (paths ending in
 * y's last token); tot = logaddexp(pb, pnb).  Start: the empty prefix with pb = 0, pnb = -inf.  At most `beam` (1..8) hypotheses are
 * live, in slots 0 .. n-1; live prefixes are pairwise distinct AS TOKEN SEQUENCES.
 * Frame t, live slots k with last token e_k (none for the empty prefix):
 *   1. the stay candidate of slot k (flat index k V + 0): spb = tot_k + lp(t, 0); spnb = pnb_k + lp(t, e_k), -inf for the empty prefix.
 *   2. the extension of slot k by v in 1 .. V-1: x = (v == e_k ? pb_k : tot_k) + lp(t, v).  If a live slot j spells y_k + [v], the
 *      extension is folded into j's stay candidate, spnb_j = logaddexp(spnb_j, x), and is no candidate of its own (a slot receives at
 *      most one fold per frame).  Otherwise it is the candidate k V + v with pb = -inf, pnb = x.
 *   3. candidates whose total is -inf are dropped; the rest are ordered by total descending, exact float32 ties to the LOWER flat
 *      index; the first `beam` become the new slots in rank order.  With no finite candidate, slot 0's stay candidate alone survives
 *      and its scores stay -inf from then on.
 *   4. a selected extension appends v: timestamp t, token log-prob lp(t, v) -- the input value itself, the convention of
 *      k2hip_ctc_align.  A hypothesis that receives a fold keeps its own timestamps and token log-probs (the first-inserted rule).
 * After the last frame the score of a hypothesis is its tot (no length normalisation); the slots are ordered by it; entry 0 is the
 * result, the N-best the first min(nbest, live) slots.  All arithmetic is float32, logaddexp(a,b) = m + log1p(exp(min - m)); -inf
 * operands give no NaN.
 * PREFIX IDENTITY IS SEQUENCE IDENTITY.  "Slot j spells y_k + [v]" speaks of token sequences, not of history nodes: when a prefix P
 * leaves the beam while its descendant P+w stays, P is later spelled again from its parent and that new P is extended by w, the
 * extension folds into the old P+w -- two equal prefixes are never live together.
 * Not covered: vocabulary pruning, length normalisation.  Hotwords and the n-gram LM are ignored by this search unless the model opts
 * in ("Hotword and n-gram LM biasing of the CTC prefix beam search" below).  Streaming: the carried form below
 * (k2hip_ctc_prefix_beam_search_chunk).
 *
 * k2hip_ctc_prefix_beam_search: operator level.  Output shapes and the K2HIP_ERR_CAPACITY rule are those of k2hip_beam_search_nbest
 * (B = R).  K2HIP_ERR_UNSUPPORTED for a transducer model; K2HIP_ERR_INVALID for beam outside 1..8, nbest outside 1..beam, n_frames
 * outside [1, Tprime] or R outside [1, 65535], decided on the host before any device work.  Independent of the model's decoding
 * method and k2hip_set_nbest. */
int32_t k2hip_ctc_prefix_beam_search(k2hip_model_t* model, const float* log_probs, int32_t R, int32_t Tprime, const int32_t* n_frames,
                                     int32_t beam, int32_t nbest, int64_t* tokens, int32_t* timestamps, float* token_log_probs,
                                     int32_t* n_tokens, int32_t* n_hyps, float* scores, int32_t max_tokens);
/* ---- Hotword and n-gram LM biasing of the CTC prefix beam search (offline; zipformer2ctc models) ---------------------------------
 * The reference has no counterpart; the semantics are this project's own.  Everything not mentioned is the rule of "CTC prefix beam
 * search with N-best" above, unchanged.  The tables are those of k2hip_set_hotwords (dense next / bonus [S][V], pending [S]) and
 * k2hip_set_ngram_lm (the sparse automaton, every weight already multiplied by the scale).
 * SLOT STATE.  Every live slot carries three more values: hs, the hotword graph state (start 0); ls, the LM state (start: the LM's
 *   start state); ctx, the float32 accumulated context score (start 0.0f).  All three are functions of the slot's token sequence
 *   alone, ctx bit for bit: a sequence is always built by the same float32 additions in the same order, also when it is re-spelled.
 *   So the fold rule needs nothing new: a slot that receives a fold keeps its own hs, ls and ctx.  pb and pnb stay purely acoustic.
 * CANDIDATE KEYS.  Stay candidate of slot k: key st_k + ctx_k, st_k = logaddexp(spb, spnb) as above.  Extension k V + v that is not
 *   folded: cb = ctx_k + bonus[hs_k][v], key x + cb -- the hotword bonus takes part IN THE SELECTION (otherwise a biased token would
 *   have to make a beam of at most 8 unaided).  A candidate is dropped when its ACOUSTIC total is -inf, as above.  Order: key
 *   descending, exact ties to the lower flat index.  No finite candidate: slot 0's stay candidate survives alone, unchanged.
 * A SELECTED EXTENSION takes hs' = next[hs_k][v], then the LM step (term, ls') = Step(ls_k, v) over the scaled tables, and
 *   ctx' = cb + term, in that order.  The LM term is NOT in that frame's selection (as in the modified beam search); it is in every
 *   later key.  Slots stay in selection rank order.
 * UNK AND BLANK.  Unk (id 2) is an ordinary CTC token; for both automata it leaves the state alone and earns nothing (the dense
 *   hotword tables say so; the LM walk is skipped).  Blank is never appended.
 * AFTER THE LAST FRAME final_q = (tot_q + ctx_q) - pending[hs_q]: an unfinished match earns nothing; nothing is subtracted for the
 *   LM.  Entries are ordered by final descending, ties to the lower slot; entry 0 is the result; scores and k2hip_last_scores report
 *   final.  Token log-probs stay the input values lp(t, v).
 * NULL AND TRIVIAL TABLES.  Hotwords without an LM, or an LM without hotwords: the missing half contributes exactly nothing.  An
 *   empty graph, score_per_token = 0 or LM scale 0 adds +0.0f: the result is bit for bit the plain search.
 *
 * k2hip_set_ctc_prefix_biasing: the opt-in, OFF by default (then the search above ignores both tables and its results are bit for
 * bit what they always were).  On: k2hip_ctc_prefix_beam_search and the batch entries under "ctc_prefix_beam_search"
 * (k2hip_offline_greedy*, k2hip_offline_recognizer_get_results, submit / wait) use the model's hotword and LM tables; with neither
 * set the plain search runs.  K2HIP_ERR_UNSUPPORTED for a transducer model; K2HIP_ERR_INVALID with batches in flight, as for
 * k2hip_set_hotwords.  Unaffected either way: k2hip_online_step, k2hip_ctc_prefix_beam_search_chunk (the carried streaming search
 * never reads this switch nor the model-level hotword list; it has a per-stream switch of its own, below), the collapse,
 * k2hip_ctc_align. */
int32_t k2hip_set_ctc_prefix_biasing(k2hip_model_t* model, int32_t on);
/* ---- streaming CTC prefix beam search: prefixes carried across chunks (operator level) ------------------------------------------
 * A k2hip_ctc_prefix_stream_t is one stream's live prefixes (host memory; no device slot), shaped like k2hip_beam_stream_t.
 * k2hip_ctc_prefix_beam_search_chunk continues every listed stream over its next n_frames[b] (NULL = Tc) rows of log_probs
 * [B][Tc][V] -- what k2hip_online_encoder-style producers of a CTC model's log-probs deliver per chunk.  Nothing new is defined: after
 * any sequence of calls, whatever the chunk lengths and the batch composition per call, a stream's live prefixes are EXACTLY those of
 * the search above run once over the concatenation of all frames it has been given -- in rank order, each with its tokens, ABSOLUTE
 * frame timestamps, token log-probs and (pb, pnb, tot), bit for bit, the float32 scores included (both forms run the same float32
 * operations in the same order; the score has no length normalisation).  Prefix identity, the fold rule, the tie rule, the
 * first-inserted rule and the all -inf rule cross a chunk boundary unchanged.
 * create: beam 1..8, nbest 1..beam (the alternatives the stream serves), else K2HIP_ERR_INVALID; K2HIP_ERR_UNSUPPORTED for a
 * transducer model.  The chunk call fails with K2HIP_ERR_UNSUPPORTED for a transducer model and with K2HIP_ERR_INVALID for streams
 * of different beams in one call, a stream listed twice, a stream of another model, or n_frames[b] outside [1, Tc] -- all decided on
 * the host before any device work; a failed call leaves every stream as it was.  Independent of the model's decoding method and
 * k2hip_set_nbest.  num_frames: the frames searched so far.  The getters are those of k2hip_beam_stream_*: the best prefix (entry
 * 0), its score (0 before the first chunk), and the first min(nbest, live) prefixes in rank order. */
typedef struct k2hip_ctc_prefix_stream k2hip_ctc_prefix_stream_t;
int32_t k2hip_ctc_prefix_stream_create(k2hip_model_t* model, int32_t beam /* 1..8 */, int32_t nbest /* 1..beam */, k2hip_ctc_prefix_stream_t** out);
int32_t k2hip_ctc_prefix_stream_destroy(k2hip_ctc_prefix_stream_t* s);
int32_t k2hip_ctc_prefix_stream_reset(k2hip_ctc_prefix_stream_t* s);
int64_t k2hip_ctc_prefix_stream_num_frames(const k2hip_ctc_prefix_stream_t* s);
int32_t k2hip_ctc_prefix_beam_search_chunk(k2hip_model_t* model, k2hip_ctc_prefix_stream_t* const* streams, int32_t B, const float* log_probs /* [B,Tc,V] */,
                                           int32_t Tc, const int32_t* n_frames /* [B] in 1..Tc, or NULL */);
int32_t k2hip_ctc_prefix_stream_num_tokens(const k2hip_ctc_prefix_stream_t* s);
int32_t k2hip_ctc_prefix_stream_get_tokens(const k2hip_ctc_prefix_stream_t* s, int64_t* tokens, int32_t cap);
int32_t k2hip_ctc_prefix_stream_get_timestamps(const k2hip_ctc_prefix_stream_t* s, int32_t* timestamps, int32_t cap);
int32_t k2hip_ctc_prefix_stream_get_token_log_probs(const k2hip_ctc_prefix_stream_t* s, float* out, int32_t cap);
int32_t k2hip_ctc_prefix_stream_get_score(const k2hip_ctc_prefix_stream_t* s, float* score);
int32_t k2hip_ctc_prefix_stream_num_alternatives(const k2hip_ctc_prefix_stream_t* s);
int32_t k2hip_ctc_prefix_stream_get_alternative(const k2hip_ctc_prefix_stream_t* s, int32_t i, int64_t* tokens, int32_t* timestamps,
                                                float* token_log_probs, int32_t cap, int32_t* n, float* score);
/* Recognizer level: k2hip_online_stream_set_ctc_prefix_beam(s, beam, nbest) opts ONE stream of a streaming CTC model into the carried
 * prefix search (beam 1..8, nbest 1..beam the alternatives it serves; beam 0 = off, the reference's per-chunk collapse).  Per stream
 * because k2hip_set_decoding_method(model, "ctc_prefix_beam_search") covers the offline entries only -- k2hip_online_step under it
 * keeps failing with K2HIP_ERR_INVALID -- and k2hip_set_nbest on a CTC model keeps its rules.  K2HIP_ERR_UNSUPPORTED on a model without
 * a CTC head; K2HIP_ERR_INVALID for beam / nbest out of range, or once the stream has searched a chunk (legal again after
 * k2hip_online_stream_reset, which keeps the setting and drops the prefixes).
 * k2hip_online_step with such streams: every stream of the list must carry the same beam setting (0 included), else K2HIP_ERR_INVALID
 * before anything moves.  The chunk's log-probs continue the stream's prefixes in the tick's own launch sequence (the in blocks ride
 * the tick's one upload, the out blocks its one download); Tokens become [blank, blank] + the best prefix over all frames so far,
 * Timestamps its ABSOLUTE frames (as under the streaming modified beam search), n_new_tokens[i] the signed change of its length --
 * re-read Tokens, earlier ones can change.  k2hip_online_stream_get_score / _num_alternatives / _get_alternative /
 * _get_token_log_probs serve it (score 0 and one empty alternative before the first chunk).  Streams without the setting decode
 * exactly as before. */
int32_t k2hip_online_stream_set_ctc_prefix_beam(k2hip_online_stream_t* s, int32_t beam /* 0 = off, 1..8 */, int32_t nbest /* 1..beam */);
/* ---- Biasing of the streaming CTC prefix beam search -----------------------------------------------------------------------------
 * Nothing new is defined.  The semantics are those of "Hotword and n-gram LM biasing of the CTC prefix beam search" above, applied to
 * all frames a stream has been given: after any sequence of chunk calls (any chunk lengths, any batch composition per call, ragged
 * n_frames, other streams of the call biased differently or not at all) a biased stream holds EXACTLY what the offline biased search
 * holds after one run over the concatenation of its frames with the same tables -- the slots in selection-rank order, each with tokens,
 * absolute frame timestamps, token log-probs, pb, pnb, tot, ctx, hs, ls; the entries in (final desc, slot asc) order with
 * final = (tot + ctx) - pending[hs]; all of it bit for bit, the float32 ctx and final included (one per-frame source; ctx is a
 * function of the token sequence alone).
 *   What is CARRIED keeps the pending bonus: the carried ctx of a slot whose match is under way still holds that bonus, because the
 *   match may complete in the next chunk; nothing is subtracted from what is carried.
 *   The slots are carried in SELECTION-RANK order, not in final order: the tie rule "lower flat index" of the next frame depends on it.
 *   What a stream REPORTS after a step is entry 0 in final order (tokens, timestamps, token log-probs), its score final, and as
 *   alternatives the first min(nbest, live) entries in final order.  Tokens can therefore be revised from step to step more often than
 *   in the unbiased search; n_new_tokens stays a signed change: re-read Tokens after every step.
 *   Example (the flip row of tests/ctc_prefix_bias_cases.py, phrase [a, b], one frame per chunk): after frame 0 the slots are [a]
 *   (hs = 1, ctx = 1.5, pending) and [b], but the reported result is [b] with score -1.25; after frame 1 it is [a, b] with score 1.0,
 *   after frame 2 [a, b] with score 0.75 exactly.
 * The switch is PER STREAM and OFF by default: k2hip_online_stream_set_ctc_prefix_biasing (recognizer level) and
 * k2hip_ctc_prefix_stream_set_biasing (operator level).  On: the stream's carried search reads the graph attached to THAT stream, if
 * any (k2hip_online_stream_set_hotwords / k2hip_ctc_prefix_stream_set_hotwords; uploads are shared between streams of one model as
 * for the beam streams), and the model's n-gram LM of k2hip_set_ngram_lm, if one is set when the stream searches its first chunk.
 * Off: both are ignored, the results are bit for bit the unbiased search's; an attached graph stays ignored.  The model-level list of
 * k2hip_set_hotwords and k2hip_set_ctc_prefix_biasing never apply to streaming.
 * The three setters are legal only while the stream holds the start state -- before its first searched chunk, or after a reset --
 * else K2HIP_ERR_INVALID ("... reset the stream first").  A reset keeps the switch and the graph and returns every prefix to hs = 0,
 * ctx = 0, ls = the start state of the LM then set.  K2HIP_ERR_UNSUPPORTED on a model without a CTC head; the graph's vocab_size is
 * checked against the model.
 * The LM follows the rule of the streaming beam search: a biased stream keeps the setting it searched its first chunk with; after
 * k2hip_set_ngram_lm changed or cleared it, a chunk call or k2hip_online_step naming that stream fails with K2HIP_ERR_INVALID and no
 * stream changes; a change that lands between the checks and the launch is caught under the launch's lock ("... call again").
 * Streams with the switch off are not subject to the rule.
 * One call may mix biased and unbiased streams, different graphs, graph-only, LM-only and both.  A call in which no stream is biased
 * issues the unbiased launch, unchanged.  Otherwise the biased kernel runs for the whole call: streams without a graph get null
 * tables, streams that do not run the LM have it masked off, and their results are bit for bit the plain search's.  Every stream of
 * one call still carries the same beam setting. */
int32_t k2hip_online_stream_set_ctc_prefix_biasing(k2hip_online_stream_t* s, int32_t on);
int32_t k2hip_ctc_prefix_stream_set_hotwords(k2hip_ctc_prefix_stream_t* s, const k2hip_hotwords_t* hw /* NULL: detach */);
int32_t k2hip_ctc_prefix_stream_set_biasing(k2hip_ctc_prefix_stream_t* s, int32_t on);
/* Per stream.  num_alternatives: the count (>= 1; -1 for NULL, for online streams a negative error code under greedy_search).
 * get_alternative(i): tokens / timestamps / token_log_probs [cap] (each may be NULL), *n = its length, *score = its finalized
 * log-prob; K2HIP_ERR_CAPACITY if cap is too small (nothing is written), K2HIP_ERR_INVALID for i outside the list.
 * get_token_log_probs: those of the best result, parallel to its timestamps; returns the count, or a negative error code
 * (K2HIP_ERR_CAPACITY: nothing written).  Offline streams: alternatives' timestamps are frame indexes of the utterance, tokens carry
 * no seed prefix. */
int32_t k2hip_offline_stream_num_alternatives(const k2hip_offline_stream_t* s);
int32_t k2hip_offline_stream_get_alternative(const k2hip_offline_stream_t* s, int32_t i, int64_t* tokens, int32_t* timestamps,
                                             float* token_log_probs, int32_t cap, int32_t* n, float* score);
int32_t k2hip_offline_stream_get_token_log_probs(const k2hip_offline_stream_t* s, float* out, int32_t cap);
int32_t k2hip_online_stream_num_alternatives(const k2hip_online_stream_t* s);
int32_t k2hip_online_stream_get_alternative(const k2hip_online_stream_t* s, int32_t i, int64_t* tokens, int32_t* timestamps,
                                            float* token_log_probs, int32_t cap, int32_t* n, float* score);
int32_t k2hip_online_stream_get_token_log_probs(const k2hip_online_stream_t* s, float* out, int32_t cap);
int32_t k2hip_beam_stream_num_alternatives(const k2hip_beam_stream_t* s);
int32_t k2hip_beam_stream_get_alternative(const k2hip_beam_stream_t* s, int32_t i, int64_t* tokens, int32_t* timestamps,
                                          float* token_log_probs, int32_t cap, int32_t* n, float* score);
int32_t k2hip_beam_stream_get_token_log_probs(const k2hip_beam_stream_t* s, float* out, int32_t cap);

/* OfflineRecognizer.GetResults (:85-91) minus DecodeMulti: runs the fused batch
 * path on the streams' feature buffers, stores Tokens/Timestamps in each stream
 * (including the reference's 2*B-blank prefix) and calls RemoveSamples (:294). */
int32_t k2hip_offline_recognizer_get_results(k2hip_model_t* model, k2hip_offline_stream_t* const* streams, int32_t B);
/* OfflineRecognizer.GetResult (:77-83): single-stream path, Tokens = [-1, blank, ...] */
int32_t k2hip_offline_recognizer_get_result(k2hip_model_t* model, k2hip_offline_stream_t* stream);
/* stream.Tokens / stream.Timestamps exactly as the reference would hold them */
int32_t k2hip_offline_stream_num_tokens(const k2hip_offline_stream_t* s);
int32_t k2hip_offline_stream_num_timestamps(const k2hip_offline_stream_t* s);
int32_t k2hip_offline_stream_get_tokens(const k2hip_offline_stream_t* s, int64_t* tokens, int32_t cap);
int32_t k2hip_offline_stream_get_timestamps(const k2hip_offline_stream_t* s, int32_t* timestamps, int32_t cap);

/* ======================= streaming path: OnlineRecognizer / IOnlineProj ==========================
 * The reference's IOnlineProj (IOnlineProj.cs:65-71) exposes GetEncoderInitStates / stack_states /
 * unstack_states / EncoderProj(x, states): per tick it copies every stream's ~1.85 MB of caches into
 * batch-major ONNX inputs and back on the host (OnlineProjOfZipformer2.cs:144-489).  Here a stream's
 * caches live in a slot of a device-resident pool for the stream's whole life, so the drop-in unit is
 * the stream handle + one step call; stack/unstack have no counterpart (nothing is copied).
 * NB: for B > 1 the reference's stack_states mis-strides cached_nonlin_attn (:254-262 vs :407-413) and
 * mixes streams; this engine keeps streams independent, i.e. it reproduces the reference at B = 1. */

/* OnlineStream ctor (OnlineStream.cs:22-47): GetEncoderInitStates (zeroed caches), Hyp = Tokens =
 * [blank, blank]. */
int32_t k2hip_online_stream_create(k2hip_model_t* model, k2hip_online_stream_t** out);
int32_t k2hip_online_stream_destroy(k2hip_online_stream_t* s);
/* the stream as if freshly created (caches zeroed in its slot; FIFO, tokens, timestamps, Hyp cleared).  No reference counterpart: a
 * host would create a new OnlineStream (OnlineRecognizer.cs:60-64); SURVEY 8b lists it as a convenience of the C surface. */
int32_t k2hip_online_stream_reset(k2hip_online_stream_t* s);
/* ChunkLength = T, ShiftLength = decode_chunk_len (OnlineModel.cs:48-49); frames of encoder_out per chunk */
int32_t k2hip_online_chunk_info(const k2hip_model_t* model, int32_t* chunk_length, int32_t* shift_length,
                                int32_t* frames_per_chunk);
/* OnlineStream.AddSamples (:57-79): streaming fbank on the new samples, frames appended to the FIFO */
int32_t k2hip_online_stream_accept_samples(k2hip_online_stream_t* s, const float* samples, int64_t n);
/* AddSamples for many streams at once (one fbank launch for the whole round when every stream is at the
 * same position, e.g. a server that feeds all connections on a common tick; falls back to per-stream
 * launches otherwise).  Semantically B independent AddSamples calls. */
int32_t k2hip_online_accept_samples_batch(k2hip_model_t* model, k2hip_online_stream_t* const* streams, int32_t B,
                                          const float* const* samples, const int64_t* n);
/* ... or push ready-made feature frames ([n_frames, feature_dim]) */
/* the same over the rows of one [B, n] sample matrix (row_stride in floats) */
int32_t k2hip_online_accept_samples_matrix(k2hip_model_t* model, k2hip_online_stream_t* const* streams, int32_t B, const float* samples,
                                           int64_t row_stride, int64_t n);
int32_t k2hip_online_stream_accept_features(k2hip_online_stream_t* s, const float* feats, int64_t n_frames);

/* ---- Input at other sample rates --------------------------------------------------------------------------------------------------
 * The accept_samples entries take samples at the model's rate (k2hip_model_info.sample_rate).  The accept_waveform entries take
 * (sample_rate, samples) and convert on the device: Kaldi's LinearResample written from its definition, a Hann-windowed sinc with 6
 * zero crossings and cutoff 0.99 * 0.5 * min(in, out), without flush -- an output sample exists once its whole window has been
 * accepted, so the last <= 6 / (0.99 min(in, out)) seconds of a stream (under 0.4 ms towards 16 kHz; less than a frame shift) stay
 * withheld.  Output k = u * ou + p (iu : ou = in : out in lowest terms) is sum_j w[p][j] * x[first[p] + u * iu + j] in float32, taps
 * ascending by fused multiply-add from +0; x is zero in front of the stream's first sample.  Any chunking of a stream gives the same
 * bits.
 * Rules: sample_rate equal to the model's is exactly accept_samples (no plan, no launch, same bits).  A stream's rate is fixed by
 * its first samples -- an offline stream's for its lifetime, an online stream's until k2hip_online_stream_reset; samples at another
 * rate later, or accept_samples on a stream that resamples, return K2HIP_ERR_INVALID with the two rates in the message.
 * Refusals: sample_rate <= 0 is K2HIP_ERR_INVALID; a pair of rates whose filter table (out / gcd phases x taps) exceeds 65536 floats
 * (16001 -> 16000) or has more than 256 taps per phase is K2HIP_ERR_UNSUPPORTED, the message names the two rates.
 * An offline stream queues its raw samples in pinned memory as ever (no launch, no lock on the model); SpeechLength counts the
 * frames of the samples the queue will give, and k2hip_offline_recognizer_get_results converts the whole batch, any mix of rates,
 * in the one launch that gathers it.  An online stream converts when its frames are needed, all streams of a step in one launch.
 * k2hip_resample_num_out: samples at the model's rate that n_in_total samples at in_rate give in all (-1 on error).
 * k2hip_resample: one call over a whole signal (no flush, no state): *n_out = k2hip_resample_num_out(n) samples into out;
 * K2HIP_ERR_CAPACITY when cap is short (*n_out is set, nothing is written). */
int64_t k2hip_resample_num_out(k2hip_model_t* model, int32_t in_rate, int64_t n_in_total);
int32_t k2hip_resample(k2hip_model_t* model, int32_t in_rate, const float* samples, int64_t n, float* out, int64_t cap, int64_t* n_out);
int32_t k2hip_offline_stream_accept_waveform(k2hip_offline_stream_t* s, int32_t sample_rate, const float* samples, int64_t n);
int32_t k2hip_online_stream_accept_waveform(k2hip_online_stream_t* s, int32_t sample_rate, const float* samples, int64_t n);
/* B k2hip_online_stream_accept_waveform calls at one rate */
int32_t k2hip_online_accept_waveform_batch(k2hip_model_t* model, k2hip_online_stream_t* const* streams, int32_t B, int32_t sample_rate,
                                           const float* const* samples, const int64_t* n);
/* OnlineInputEntity.SpeechLength (floats buffered) */
int64_t k2hip_online_stream_speech_length(const k2hip_online_stream_t* s);
/* copies the buffered frames to out (cap floats; K2HIP_ERR_CAPACITY if short); the frames of samples accepted earlier are computed first */
int32_t k2hip_online_stream_get_speech(k2hip_online_stream_t* s, float* out, int64_t cap);
/* OnlineStream.IsFinished(isEndpoint) (:124-161), including its side effect of feeding 400 zero
 * samples when less than a chunk is buffered */
int32_t k2hip_online_stream_is_finished(k2hip_online_stream_t* s, int32_t is_endpoint, int32_t* finished);
/* OnlineRecognizer.GetResults -> ForwardBatchGreedySearch (OnlineRecognizer.cs:76-219), minus DecodeMulti:
 * every stream with a full chunk buffered (GetDecodeChunk :82-100) is decoded for that chunk
 * (RemoveChunk :102-117 drops ShiftLength frames), its Hyp / Tokens / Timestamps / caches are updated;
 * decoded[i] = 1 for those, 0 for streams that had no chunk (the reference removes them from the
 * caller's list, :117-120); n_new_tokens[i] = symbols emitted in this chunk.
 * Under modified_beam_search (k2hip_set_decoding_method) the chunk continues the stream's beam search instead: Tokens /
 * Timestamps / Hyp become the best hypothesis over all frames so far (absolute timestamps), n_new_tokens[i] is the signed change
 * of its length -- re-read Tokens, earlier ones can change -- and a stream whose method or beam changed since its first chunk
 * fails the call with K2HIP_ERR_INVALID until it is reset.
 * On failure no stream's host-side state has moved (no chunk removed, no token appended), but the DEVICE caches of the streams
 * that were being decoded may have advanced in place; those streams are marked and every later k2hip_online_step that names one
 * returns K2HIP_ERR_INVALID until k2hip_online_stream_reset -- the same chunk is never fed into caches that already moved. */
int32_t k2hip_online_step(k2hip_model_t* model, k2hip_online_stream_t* const* streams, int32_t B, int32_t* decoded,
                          int32_t* n_new_tokens);
/* the stream's processed_lens state as the reference holds it between steps (Zipformer2: frames consumed; Conformer: 2 at
 * creation, then the batch size of its last step -- OnlineProjOfConformer.cs:77,229) */
/* ---- operator level of the streaming path: IOnlineProj (IOnlineProj.cs:65-71) ----------------------------------------
 * For a host that keeps the reference's OnlineRecognizer loop unchanged and swaps only the operator (csharp/OnlineProjOfHip.cs).
 * A k2hip_online_state_t is ONE stream's encoder caches: a slot of the device state pool plus processed_lens.  It replaces the
 * List<List<float[]>> of GetEncoderInitStates (OnlineProjOfZipformer2.cs:144-238); stack_states / unstack_states (:240-489)
 * are the identity on handles because EncoderProj advances the caches in place.  Streaming Zipformer2 models: transducer, and
 * zipformer2ctc, whose EncoderProj output is [B, T', V] log-probs (the CTC head and the row log-softmax are part of the encoder entry;
 * k2hip_model_info.reserved reports the width) -- the producer of k2hip_ctc_prefix_beam_search_chunk. */
typedef struct k2hip_online_state k2hip_online_state_t;
int32_t k2hip_online_state_create(k2hip_model_t* model, k2hip_online_state_t** out);
int32_t k2hip_online_state_destroy(k2hip_online_state_t* state);
int64_t k2hip_online_state_processed_len(const k2hip_online_state_t* state);
/* EncoderProj (OnlineProjOfZipformer2.cs:491-618): feats [B, ChunkLength, FeatureDim] raw fbank frames (OnlineInputEntity.Speech of
 * each stream's GetDecodeChunk), encoder_out [B, T', joiner_dim] (T' = k2hip_online_chunk_info's frames_per_chunk).  Decoder and
 * joiner are k2hip_decoder / k2hip_joiner.  K2HIP_ERR_CAPACITY if cap_floats is too small (checked before any work: nothing
 * advances).  If the device work itself fails, processed_lens does not advance but the states' caches may have been updated in
 * place: those states are marked, later calls that name one return K2HIP_ERR_INVALID; destroy and re-create them. */
int32_t k2hip_online_encoder(k2hip_model_t* model, k2hip_online_state_t* const* states, int32_t B, const float* feats, float* encoder_out,
                             int64_t cap_floats);

int64_t k2hip_online_stream_processed_len(const k2hip_online_stream_t* s);
int32_t k2hip_online_stream_num_tokens(const k2hip_online_stream_t* s);
int32_t k2hip_online_stream_num_timestamps(const k2hip_online_stream_t* s);
int32_t k2hip_online_stream_get_tokens(const k2hip_online_stream_t* s, int64_t* tokens, int32_t cap);
int32_t k2hip_online_stream_get_timestamps(const k2hip_online_stream_t* s, int32_t* timestamps, int32_t cap);
int32_t k2hip_online_stream_get_hyp(const k2hip_online_stream_t* s, int64_t* hyp2);
/* log-prob of the best hypothesis of a stream under modified_beam_search (0 before its first chunk); K2HIP_ERR_INVALID for a
 * stream that decodes with greedy_search */
int32_t k2hip_online_stream_get_score(const k2hip_online_stream_t* s, float* score);
/* copy one cache out of the stream's device slot (parity tests / debugging):
 * kind 0 cached_key [left,32H], 1 cached_nonlin_attn [left,3D/4], 2/3 cached_val1/2 [left,12H],
 * 4/5 cached_conv1/2 [D,K/2], 6 embed_states [128,3,19] (layer ignored); out == NULL queries n.
 * For an "lstm" model (OnlineProjOfLstm.cs:55-75): kind 0 = h of `layer` [d_model], kind 1 = c of `layer` [rnn_hidden_size];
 * for a streaming "conformer" (OnlineProjOfConformer.cs:55-82): kind 0 = cached_attn of `layer` [left_context, D], kind 1 =
 * cached_conv of `layer` [K-1, D] */
int32_t k2hip_online_stream_state(k2hip_online_stream_t* s, int32_t layer, int32_t kind, float* out, int64_t cap, int64_t* n);

/* ---- Voice activity detection and long recordings ---------------------------------------------------------------------------------
 * No reference counterpart: the reference has only IsFinished(isEndpoint) and is fed pre-cut files.  The detector works on what the
 * engine computes anyway, the log-mel features, so a segment is a range of rows of a feature matrix and its transcript is exactly
 * what the offline entries give for the same samples.  Everything is counted in fbank frames (the model's frame_shift_ms and
 * frame_length_ms: 160 and 400 samples at 16 kHz in every preset); the normative text is csrc/vad_ref.h, DESIGN.md "Voice activity
 * detection and long recordings" the prose.
 * Per frame t of a stream, numbered from its start or its last reset:
 *   s_t = float32 mean of x[t][band_lo .. band_hi) in vad_ref.h's fixed order, m_t = the mean of s_{t-4} .. s_t (s_u := s_0 for u < 0,
 *   summed left to right, times 0.2f), n_t = min over the last floor_window frames u of m_u + rise * (float)(t - u) (product and sum
 *   rounded separately), d_t = (m_t - n_t > margin) && (m_t > abs_floor).
 * A segment opens at the first speech frame, closes after min_silence frames of silence (dropped if shorter than min_speech), and is
 * cut by force once it holds max_speech frames: at the frame with the smallest m among the last max_speech / 2, the earliest on ties.
 * Reported segments [start, end) carry speech_pad frames on each side, clipped by the previous segment's end, by frame 0 and -- at
 * a flush -- by the stream's length; a forced cut gets no padding on either side.  Samples of a segment:
 * [start * frame_shift, (end - 1) * frame_shift + frame_len).  Any chunking of a stream gives the same bits.
 * The level defaults (rise 0.002, margin 2.0, abs_floor -12.0; natural-log power units, the unit of the features) are UNTUNED:
 * nobody has measured them on real speech.  The other defaults: floor_window 1000, min_silence 50, min_speech 25, speech_pad 10,
 * max_speech 2000, and the mel bins whose centre frequency lies in [300, 3500] Hz.
 * Refused with K2HIP_ERR_INVALID, the field named: band_lo >= band_hi or outside the feature row, floor_window < 8,
 * min_silence < 2 * speech_pad, max_speech < 2 * min_speech, max_speech / 2 > floor_window, a count <= 0, a level that is not
 * finite; with K2HIP_ERR_UNSUPPORTED: floor_window > 1024. */
typedef struct k2hip_vad_config {
    int32_t band_lo, band_hi;   /* mel bins [lo, hi) */
    int32_t floor_window;       /* W */
    float rise, margin, abs_floor;
    int32_t min_silence, min_speech, speech_pad, max_speech;
} k2hip_vad_config;
typedef struct k2hip_vad_stream k2hip_vad_stream_t;
int32_t k2hip_vad_default_config(const k2hip_model_t* model, k2hip_vad_config* cfg);
int32_t k2hip_vad_stream_create(k2hip_model_t* model, const k2hip_vad_config* cfg, k2hip_vad_stream_t** out);
int32_t k2hip_vad_stream_destroy(k2hip_vad_stream_t* s);
/* the stream as if freshly created: frames, carried state, queued samples, sample rate and unread segments are dropped */
int32_t k2hip_vad_stream_reset(k2hip_vad_stream_t* s);
/* end of audio: an open segment is closed and reported (its padded end clipped to the stream's length); samples short of a frame
 * are dropped; then the stream is as after a reset, except that the reported segments stay until they are popped */
int32_t k2hip_vad_stream_flush(k2hip_vad_stream_t* s);
/* feats[b]: n_frames[b] rows of feature_dim floats for streams[b]; 0 leaves a stream untouched.  One batched call on the device. */
int32_t k2hip_vad_accept_features_batch(k2hip_model_t* model, k2hip_vad_stream_t* const* streams, const float* const* feats,
                                        const int64_t* n_frames, int32_t B);
/* samples[b]: n[b] samples at sample_rate for streams[b].  fbank runs on the device and the features never leave it; a stream carries
 * the samples behind its last whole frame shift, as an online stream does.  A sample_rate other than the model's goes through the
 * resampler under the rules of "Input at other sample rates": a stream's rate is fixed by its first samples until a reset or flush. */
int32_t k2hip_vad_accept_samples_batch(k2hip_model_t* model, k2hip_vad_stream_t* const* streams, int32_t sample_rate,
                                       const float* const* samples, const int64_t* n, int32_t B);
/* 1 while a segment is open (the machine's `trig`), 0 otherwise; -1 on a null stream */
int32_t k2hip_vad_stream_is_speech(const k2hip_vad_stream_t* s);
/* frames taken since the stream's start, reset or flush */
int64_t k2hip_vad_stream_num_frames(const k2hip_vad_stream_t* s);
/* reported segments not popped yet, oldest first */
int32_t k2hip_vad_stream_num_segments(const k2hip_vad_stream_t* s);
int32_t k2hip_vad_stream_get_segments(const k2hip_vad_stream_t* s, int64_t* start, int64_t* end, int32_t* forced, int32_t cap);
int32_t k2hip_vad_stream_pop_segments(k2hip_vad_stream_t* s, int32_t n);
/* A long recording in one call: fbank over all of it into a resident block on the device (32 KB per second of audio), the detector
 * and its flush, the segments packed in order into batches -- a batch closes at max_batch segments, or when (count + 1) * longest
 * frames would exceed max_batch_frames; a segment longer than that on its own is a batch of one --, each batch gathered device to
 * device and decoded by the model's current offline search exactly as k2hip_offline_recognizer_get_results runs it, the best
 * hypothesis kept.  Timestamps are segment-local encoder frames; the segment's frame range goes with them, and `batch` names the
 * batch it was decoded in (the offline encoder does not mask padding: a segment's tokens are those of k2hip_offline_greedy_from_samples
 * on the sample ranges of its batch).  cfg == NULL: the defaults.  A recording of more than 2^27 samples at the model's rate (2 h 19 min
 * at 16 kHz) is refused with K2HIP_ERR_UNSUPPORTED.  A sample_rate other than the model's is resampled first. */
typedef struct k2hip_long_result k2hip_long_result_t;
int32_t k2hip_offline_recognize_long(k2hip_model_t* model, int32_t sample_rate, const float* samples, int64_t n, const k2hip_vad_config* cfg,
                                     int32_t max_batch, int64_t max_batch_frames, k2hip_long_result_t** result);
int32_t k2hip_long_result_num_segments(const k2hip_long_result_t* r);
int32_t k2hip_long_result_get_segment(const k2hip_long_result_t* r, int32_t i, int64_t* start, int64_t* end, int32_t* forced, int32_t* batch);
/* *n = the segment's token count; K2HIP_ERR_CAPACITY when cap is short (nothing is written) */
int32_t k2hip_long_result_get_tokens(const k2hip_long_result_t* r, int32_t i, int64_t* tokens, int32_t* timestamps, int32_t cap, int32_t* n);
int32_t k2hip_long_result_destroy(k2hip_long_result_t* r);

/* ---- Neural LM rescoring: LSTM language model scores for N-best lists ------------------------------------------------------------
 * (no reference counterpart; the toolkit the searches follow rescores with an icefall RnnLmModel: embedding -> multi-layer LSTM ->
 * linear -> log_softmax.  The normative text is csrc/rnn_lm_ref.h, DESIGN.md "Neural LM rescoring".)
 * THE LM is a .k2w container: metadata model_type=rnn_lm, vocab_size (V), embedding_dim (E), hidden_dim (H), num_layers (L, 1..8),
 * sos_id, eos_id (icefall: both 1), tie_weights (0/1); tensors under their icefall / torch state-dict names in torch layout:
 * input_embedding.weight [V,E]; rnn.weight_ih_l{k} [4H,in] (in = E for k = 0, else H), rnn.weight_hh_l{k} [4H,H], rnn.bias_ih_l{k} and
 * rnn.bias_hh_l{k} [4H]; output_linear.weight [V,H], output_linear.bias [V].  With tie_weights=1 output_linear.weight may be absent:
 * it is then the embedding, which needs E == H.  Gate order is torch's (i, f, g, o); there is no projection.
 * Load refuses with K2HIP_ERR_UNSUPPORTED when H % 32 != 0 or E % 4 != 0, and with K2HIP_ERR_INVALID, naming the tensor, for a missing
 * tensor, a tensor of the wrong shape, a non-f32 tensor, a non-finite value, and sos_id / eos_id outside [0,V).
 * SCORE of one hypothesis y_1 .. y_n (ids in [0,V), n >= 0): the inputs are x = [sos, y_1 .. y_n]; the targets are [y_1 .. y_n, eos]
 * with_eos (n + 1 positions), otherwise the first n of those (n positions; n = 0: the total is 0 and no device work is issued).  The
 * layers start from h = c = 0.  At position t, layer k: gates = (x_t . W_ih^T + (b_ih + b_hh)) + h_{t-1} . W_hh^T (the two biases
 * summed once in float32 at load); c = sigmoid(f) c + sigmoid(i) tanh(g); h = sigmoid(o) tanh(c);
 * lp_t = log_softmax(h^{L-1}_t . W_out^T + b_out)[target_t]; total = the float32 sum of lp_t in position order.  All arithmetic is
 * float32.  The device is held to a float64 twin within a measured bound, not bit for bit: its expf / tanhf and the GEMM plan's
 * summation order differ from the host's, so a hypothesis' last bits may depend on what else is in the call (the caveat the offline
 * encoder carries).
 * A k2hip_rnn_lm_t belongs to no model and needs no GPU. */
typedef struct k2hip_rnn_lm k2hip_rnn_lm_t;
#define K2HIP_RNN_LM_MAX_ROWS (1 << 22) /* positions of all hypotheses of one scoring call */
int32_t k2hip_rnn_lm_load(const char* path, k2hip_rnn_lm_t** out);
int32_t k2hip_rnn_lm_destroy(k2hip_rnn_lm_t* lm);
int32_t k2hip_rnn_lm_vocab_size(const k2hip_rnn_lm_t* lm);      /* -1 for NULL, as the next five */
int32_t k2hip_rnn_lm_embedding_dim(const k2hip_rnn_lm_t* lm);
int32_t k2hip_rnn_lm_hidden_dim(const k2hip_rnn_lm_t* lm);
int32_t k2hip_rnn_lm_num_layers(const k2hip_rnn_lm_t* lm);
int32_t k2hip_rnn_lm_sos_id(const k2hip_rnn_lm_t* lm);
int32_t k2hip_rnn_lm_eos_id(const k2hip_rnn_lm_t* lm);
/* the host reference (csrc/rnn_lm_ref.h), no GPU: Hn hypotheses back to back in tokens, hypothesis i at [offsets[i], offsets[i + 1]);
 * token_log_probs (may be NULL) packed per hypothesis with its positions back to back; totals [Hn].  K2HIP_ERR_INVALID, naming the
 * hypothesis, for an id outside [0,V) and for decreasing offsets. */
int32_t k2hip_rnn_lm_score_host(const k2hip_rnn_lm_t* lm, const int64_t* tokens, const int64_t* offsets, int32_t Hn, int32_t with_eos,
                                float* token_log_probs, float* totals);
/* lm = NULL clears; scale finite and >= 0.  Checks vocab_size against the model and uploads the weights in the layouts the kernels
 * want; the model keeps its own copy, so lm may be destroyed afterwards.  Not while submitted batches are in flight.
 * RESCORING: while an LM with scale > 0 is set and k2hip_set_nbest(n > 1) is on, k2hip_offline_recognizer_get_results rescores each
 * stream's list -- under modified_beam_search on a transducer model and under ctc_prefix_beam_search on a CTC model.  All alternatives
 * of all streams go through ONE scoring call with_eos = 1; the list is then stably re-ordered by the method's own ordering quantity
 * with the score replaced by score + scale * lm_total (the float32 product rounded, then the sum): transducer
 * (score_i + scale lm_i) / (n_i + 2), CTC prefix score_i + scale lm_i.  Entry 0 becomes the stream's result (tokens, timestamps, token
 * log-probs); an alternative's reported score stays the search's own, and k2hip_offline_stream_get_alternative_lm_score gives its
 * lm_total (0 when nothing was rescored).  With n = 1 there is nothing to rescore and the LM changes nothing.
 * Everything else ignores the LM: greedy search, the plain CTC search, the single-stream k2hip_offline_recognizer_get_result, the
 * pipelined submit / wait, every streaming entry and k2hip_offline_recognize_long.  No LM, a cleared LM and scale = 0: bit for bit the
 * plain results from the plain launches.  Hotwords and the n-gram LM keep working as they do; the neural term is added on top of
 * whatever score the search reports. */
int32_t k2hip_set_rnn_lm(k2hip_model_t* model, const k2hip_rnn_lm_t* lm, float scale);
/* the device operator on the attached LM (any scale): the arguments and results of k2hip_rnn_lm_score_host, results in the caller's
 * order.  Checked on the host before any device work, K2HIP_ERR_INVALID naming the hypothesis: an id outside [0,V), decreasing
 * offsets, no LM attached, more than K2HIP_RNN_LM_MAX_ROWS positions. */
int32_t k2hip_rnn_lm_score(k2hip_model_t* model, const int64_t* tokens, const int64_t* offsets, int32_t Hn, int32_t with_eos,
                           float* token_log_probs, float* totals);
int32_t k2hip_offline_stream_get_alternative_lm_score(const k2hip_offline_stream_t* s, int32_t i, float* lm_total);

/* ---- Neural LM shallow fusion in the offline modified beam search -------------------------------------------------------------------
 * (no reference counterpart; the project's own semantics after icefall's modified_beam_search_lm_shallow_fusion.  DESIGN.md "Neural LM
 * shallow fusion"; the LM is the one of k2hip_set_rnn_lm, defined in csrc/rnn_lm_ref.h.)
 * on != 0 switches the mode on; off by default; K2HIP_ERR_INVALID while submitted batches are in flight.  With fusion off nothing
 * changes anywhere: rescoring as above, the same launches, bit for bit the same results.
 * Fusion is ACTIVE when it is on and an LM with scale > 0 is attached.  Then, wherever the offline modified beam search runs
 * (k2hip_beam_search, k2hip_beam_search_nbest, and the batch entries under modified_beam_search that honour k2hip_set_ngram_lm):
 * STATE AND START: every hypothesis carries an LM state -- (h, c) of all L layers for its token sequence without the [blank, blank]
 * prefix -- and the LM's next-token log-probs q = log_softmax(h^{L-1} W_out^T + b_out) over V.  The start hypothesis has the state
 * after sos from h = c = 0 (the first position of csrc/rnn_lm_ref.h).
 * SELECTION AND THE LM TERM: a frame's top-`beam` selection uses the same sums as without the LM.  A selected candidate of parent p that
 * appends a real token v then gets ((sum + hotword bonus) + n-gram term) + fl32(scale * q_p[v]); the merge of equal sequences follows,
 * exactly where the n-gram term is added.  Blank and unk earn nothing and keep the parent's state; the child's state is the parent's
 * advanced by v.
 * FINAL PICK AND SCORES: no eos term is applied at the end.  The final pick and all reported scores include the LM terms; token
 * log-probs and the beam trace stay acoustic.  So for a returned hypothesis y the sum of its LM terms is
 * scale * k2hip_rnn_lm_score(y, with_eos = 0) up to rounding.
 * RESCORING WHILE FUSION IS ACTIVE: k2hip_offline_recognizer_get_results does NOT also rescore (the LM would count twice), and
 * k2hip_offline_stream_get_alternative_lm_score gives 0.
 * Fusion works together with hotwords, the n-gram LM and N-best.  Greedy search, the CTC searches,
 * k2hip_offline_recognizer_get_result, the pipelined submit / wait, every streaming entry and k2hip_offline_recognize_long ignore the
 * switch: a streaming call on a model with fusion on runs the unfused search (the streaming search has a switch of its own,
 * k2hip_set_rnn_lm_stream_fusion below).
 * The device is held to a float64 twin within a bound, not bit for bit: the caveat rescoring carries. */
int32_t k2hip_set_rnn_lm_fusion(k2hip_model_t* model, int32_t on);

/* ---- Neural LM shallow fusion in the streaming modified beam search ------------------------------------------------------------------
 * (no reference counterpart; DESIGN.md "Neural LM shallow fusion in the streaming search".)
 * on != 0 switches the mode on; per model, off by default, SEPARATE from k2hip_set_rnn_lm_fusion (which no streaming entry reads).
 * Fusion is ACTIVE when this switch is on and an LM with scale > 0 is attached (k2hip_set_rnn_lm).  With it off, scale 0 or no LM every
 * streaming call issues the launches and gives the results of before, bit for bit.
 * WHERE: k2hip_beam_search_chunk, and k2hip_online_step on streams under modified_beam_search.  Every hypothesis of a stream carries the
 * LM's state from chunk to chunk (device memory owned by the model, one block per fused stream, taken with the stream's first fused chunk).
 * INVARIANT: after any chunking a stream holds what the offline fused search above gives over all frames so far -- tokens, timestamps,
 * the number and order of alternatives, scores: ((sum + hotword bonus) + n-gram term) + fl32(scale * q_parent[token]), then the merges.
 * No eos term.  Token log-probs stay acoustic.  It works together with per-stream hotwords, the n-gram LM and N-best.
 * A STREAM KEEPS THE SETTING OF ITS FIRST CHUNK, as it does for the n-gram LM: whether fusion was active, and then the attached LM (each
 * k2hip_set_rnn_lm call is a new setting, the same LM handle included) and the scale.  A later chunk under another setting is
 * K2HIP_ERR_INVALID ("reset the stream first"), decided for all streams of the call before any of them changes; so all streams of one
 * call are fused, or none is.  k2hip_beam_stream_reset / k2hip_online_stream_reset return the stream to the start state and give its
 * block back.  A call that fails leaves every stream, and every block, as it was; a block that cannot be allocated is K2HIP_ERR_HIP (or
 * the out-of-memory status) before any device work.
 * ORDER OF DESTRUCTION: k2hip_beam_stream_destroy and k2hip_beam_stream_reset after k2hip_model_destroy are allowed -- the model's end
 * frees every block, and a stream then only forgets its own.  (An online stream still has to go before its model, as before.) */
int32_t k2hip_set_rnn_lm_stream_fusion(k2hip_model_t* model, int32_t on);

/* ---- LODR: low-order density ratio beside the neural LM ------------------------------------------------------------------------------
 * (no reference counterpart; the project's own semantics after icefall's modified_beam_search_LODR / modified_beam_search_lm_rescore_LODR
 * and sherpa's lodr_fst / lodr_scale.  DESIGN.md "LODR".)  A low-order n-gram LM, usually a bi-gram trained on the acoustic model's own
 * training text, stands in for the transducer's internal LM: its score is SUBTRACTED wherever the neural LM's is added.  It is a second
 * automaton slot with a state of its own per hypothesis, beside the one of k2hip_set_ngram_lm (whose behaviour is unchanged), so a
 * positive-weight n-gram LM and a LODR LM can be set at once.
 * lm = NULL clears the setting.  scale is finite and <= 0 (icefall's convention: the weight is given as a negative number); a positive
 * value is K2HIP_ERR_INVALID -- an added n-gram weight is k2hip_set_ngram_lm's job; scale = 0 means "none".  Checks vocab_size against
 * the model and uploads the sparse automaton with every weight multiplied by scale ONCE on the host in float32 (the device only adds);
 * the model keeps its own copy, so lm may be destroyed afterwards.  K2HIP_ERR_INVALID while submitted batches are in flight.
 * LODR IS ACTIVE ONLY WHERE THE NEURAL LM ACTS: in a fused offline search (k2hip_set_rnn_lm_fusion on and an LM with scale > 0
 * attached), in a fused streaming search (k2hip_set_rnn_lm_stream_fusion), and in the rescoring k2hip_offline_recognizer_get_results
 * does.  Everywhere else the setting is ignored: the plain modified beam search, greedy search, the CTC searches' own scoring,
 * k2hip_offline_recognizer_get_result, the pipelined submit / wait and k2hip_offline_recognize_long.  With the setting ignored, with no
 * LODR LM, a cleared one and scale = 0 every call issues the launches of before and gives the same bits.
 * FUSION: every hypothesis carries a LODR state beside its n-gram state; the start hypothesis has the LODR LM's start state.  A frame's
 * top-`beam` selection uses the same sums as before.  A selected candidate of parent p that appends a real token v gets
 *   (((sum + hotword bonus) + n-gram term) + fl32(scale_nlm * q_p[v])) + Step_lodr(state_p, v)
 * where Step is the n-gram step of k2hip_set_ngram_lm over the LODR LM's scaled tables -- float32, back-off weights first and then the
 * arc, in exactly the order stated there; the merge of equal sequences follows.  Blank and unk earn nothing and keep the state.  No
 * end-of-sentence term is applied.  The final pick and all reported scores include the LODR terms; token log-probs and the beam trace
 * stay acoustic.
 * STREAMING: after any chunking a stream holds what the offline fused search with the same LODR setting gives over all frames so far;
 * the LODR state of every saved hypothesis crosses the chunk boundary.  A STREAM KEEPS THE LODR SETTING OF ITS FIRST CHUNK -- the
 * k2hip_set_lodr_lm call (every call that leaves an LM set is a new setting) and with it the scale, as for the n-gram LM; "none" where
 * the fusion is not active.  A chunk under another setting is K2HIP_ERR_INVALID ("... reset the stream first"), decided for all
 * streams of a call before anything changes; a k2hip_set_lodr_lm that lands between a call's checks and its launch is caught under the
 * lock that covers the launch.  A reset returns the hypotheses to the start state of the LODR LM then set.
 * RESCORING (transducer modified_beam_search and ctc_prefix_beam_search, wherever the neural rescoring runs): the ordering quantity
 * uses (score_i + fl32(scale_nlm * lm_i)) + lodr_i, where lodr_i is the float32 sum, in token order from the start state, of the scaled
 * steps of alternative i's tokens, computed on the host over the model's copy of the scaled automaton.  lodr_i has NO eos term (the
 * n-gram LM never has one) while the neural total keeps its with_eos = 1: the asymmetry is intended.
 * k2hip_offline_stream_get_alternative_lodr_score gives lodr_i: 0 when nothing was rescored or no LODR LM was set, and 0 while fusion
 * is active, as k2hip_offline_stream_get_alternative_lm_score does.  Reported alternative scores stay the search's own. */
int32_t k2hip_set_lodr_lm(k2hip_model_t* model, const k2hip_ngram_lm_t* lm, float scale);
int32_t k2hip_offline_stream_get_alternative_lodr_score(const k2hip_offline_stream_t* s, int32_t i, float* lodr_total);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* K2HIP_H */
