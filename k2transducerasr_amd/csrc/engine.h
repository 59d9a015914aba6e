// Engine = one model replica on one GPU: weights, HIP stream, device arena and the
// host-side orchestration of the offline path (pad -> Zipformer2 -> greedy).
#pragma once
#include <algorithm>
#include <array>
#include <condition_variable>
#include <functional>
#include <thread>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

#include "kernels.h"
#include "keywords.h"
#include "model.h"
#include "resample_plan.h"
#include "rnn_lm_plan.h"
#include "rnn_lm_fuse_layout.h"
#include "rnn_lm_stream_pool.h"
#include "rnn_lm_ref.h"
#include "search_out.h"
#include "vad_ref.h"

namespace k2hip {

// float offsets of one stream's caches inside its slot of the state pool (OnlineProjOfZipformer2.cs:63-111)
struct OnlineLayout {
    std::vector<long long> key, nonlin, val1, val2, conv1, conv2;  // per layer (Zipformer v1: nonlin = cached_avg, val1 = cached_val)
    std::vector<long long> clen;                                   // Zipformer v1: cached_len (one float) per layer
    std::vector<std::array<long long, 6>> sizes;                   // per layer, float counts in the reference's order
    long long embed = 0;
    long long floats_per_stream = 0;
    int nl = 0;
};

struct OfflineResult {
    std::vector<std::vector<int64_t>> tokens;   // emitted symbols per stream
    std::vector<std::vector<int32_t>> timestamps;
};

class Engine {
  public:
    Engine(const std::string& weights, const char* overrides, int device);
    ~Engine();

    const Model& model() const { return *model_; }
    std::mutex& mutex() { return mu_; }
    int device() const { return device_; }
    int search_retries() const { return search_retries_; }
    // test hook: rows of the all-contexts decoder table (0: the model has none) and how many floats of `n_samples` sampled rows
    // (+ the first, the start contexts' and the last) differ in their bits from the decoder run on those contexts
    void decoder_table_check(int n_samples, unsigned seed, long long* rows, long long* mismatched);
    hipStream_t stream() const { return stream_; }

    int encoder_out_frames(int T) const;
    int64_t fbank_num_frames(int64_t n_samples) const;

    // ---- operator-level entry points (host buffers in/out) ----
    void fbank_host(const float* samples, int64_t n, float* feats, int64_t cap_frames, int64_t* n_frames);
    // n_utts equal-length signals [n_utts, n] -> feats [n_utts, nf, feat] in one launch
    void fbank_host_batch(const float* samples, int64_t n, int n_utts, float* feats, int64_t nf);
    // the same for G signals that each arrive in two pieces ([head_g ; tail_g], n_head[g] + n_tail[g] == n for all g) and whose
    // frames go to G separate destinations: gathered straight into the pinned staging buffer and scattered straight out of it
    // (one host copy each way instead of three)
    // device mirror of the streams' feature FIFOs (see kernels.h fifo_*): rings of kFifoFrames frames per slot
    static constexpr int kFifoFrames = 512;
    void online_fifo_write(int slot, int pos, const float* feats, int64_t n_frames);  // host frames -> ring rows pos ..
    // (fifo_slots / fifo_pos: when given, the frames of signal g are also appended to slot fifo_slots[g]'s ring at fifo_pos[g] (< 0: not))
    void fbank_host_gather(const float* const* head, const int64_t* n_head, const float* const* tail, const int64_t* n_tail, int64_t n, int G,
                           float* const* dst, int64_t nf, const int* fifo_slots = nullptr, const int* fifo_pos = nullptr, bool defer = false);
    // defer = true: everything is enqueued (upload, fbank, the append to the device FIFOs, the download into pinned memory) but the
    // frames reach `dst` only in fbank_gather_finish(), which the caller runs after the next synchronisation of the stream it enqueues
    // on anyway (the chunk step's token download) -- a streaming tick then waits for the device once, not twice.  `dst` must stay
    // valid until then; at most one deferred gather is outstanding.
    void fbank_gather_finish();
    bool fbank_gather_pending() const { return fb_pending_.active; }
    void pad_host(const float* const* speech, const int64_t* n_floats, int B, int tail, float* out, int64_t cap, int64_t* L);
    void encoder_host(const float* x, int B, int T, float* enc_out, int64_t cap, int* Tp);
    void encoder_tap_host(const float* x, int B, int T, int tap, float* out, int64_t cap, int64_t* n);
    void decoder_host(const int64_t* y, int N, float* dec_out);
    void joiner_host(const float* enc, const float* dec, int N, float* logits);
    void greedy_host(const float* enc_out, int B, int Tp, bool single, int64_t* tokens, int32_t* ts, int32_t* n_tokens,
                     int max_tokens);
    // ---- forced alignment and full-sum scoring of given transcripts (align.hip; semantics in include/k2hip.h) ----
    // ids: the B targets back to back, lens [B]; n_frames [B] or null (= Tp for every stream).  Outputs (each may be null): timestamps /
    // token_log_probs [B][max_tokens], total / best [B].  The arguments are checked on the host before any device work (lattice_ref.h).
    void align_host(const float* enc_out, int B, int Tp, const int32_t* n_frames, const int64_t* ids, const int32_t* lens, int32_t* timestamps,
                    float* token_log_probs, float* total, float* best, int max_tokens);
    // offline_greedy_samples' fbank + pad + encoder with the plan's alignment as the stage behind them: encoder_out stays on the device,
    // every stream is aligned over all T' frames
    void align_samples(const float* const* samples, const int64_t* n_samples, int B, const int64_t* ids, const int32_t* lens, int32_t* timestamps,
                       float* token_log_probs, float* total, float* best, int max_tokens, int32_t* Tp_out);
    // ---- CTC forced alignment and full-sum scoring (ctc_align.hip; semantics in include/k2hip.h) ----
    // log_probs [R][Tp][V] on the host; n_frames [R] or null (= Tp); H targets back to back in ids, lens [H]; stream_of [H] names the row a
    // target is scored against, or null (H == R, the identity).  Outputs (each may be null): timestamps / end_frames / token_log_probs
    // [H][max_tokens], total / best [H].  The arguments are checked on the host before any device work (ctc_lattice_ref.h).
    void ctc_align_host(const float* log_probs, int R, int Tp, const int32_t* n_frames, int H, const int32_t* stream_of, const int64_t* ids,
                        const int32_t* lens, int32_t* timestamps, int32_t* end_frames, float* token_log_probs, float* total, float* best,
                        int max_tokens);
    // the same with the CTC plan as the stage: log_probs stay on the device, every target is aligned over all T' frames
    void ctc_align_samples(const float* const* samples, const int64_t* n_samples, int B, int H, const int32_t* stream_of, const int64_t* ids,
                           const int32_t* lens, int32_t* timestamps, int32_t* end_frames, float* token_log_probs, float* total, float* best,
                           int max_tokens, int32_t* Tp_out);
    // ---- keyword spotting: trie Viterbi on the lattice (kws.hip; semantics in include/k2hip.h "Keyword spotting") ----
    // A graph made resident: ONE device allocation [decoder rows [S][J] | the trie's tables], the rows from the decoder() launch on the
    // S contexts.  The caller owns the allocation (dev_free) and shares it among the streams of the graph.
    void* kws_graph_upload(const KeywordGraph& g, KwsGraphDev* out);
    // One stream of a chunk call: its resident graph, the T frames it takes (0: untouched) and its carried block (kws_ref.h)
    struct KwsIO {
        const KwsGraphDev* graph;
        int T;
        const float* a;
        const int32_t* start;
    };
    // What a chunk call gives back: row b of keyword / end / start / sum [B][mt] holds n[b] events, a / st the new carried blocks, stream
    // b's at state_off[b]
    struct KwsResult {
        int mt = 0;
        std::vector<int64_t> keyword;
        std::vector<int32_t> end, start, n, st, state_off;
        std::vector<float> sum, a;
    };
    // enc_out [B][Tc][J] on the host; the arguments are checked before any device work, and nothing of `io` is written
    void kws_chunk_host(const float* enc_out, int B, int Tc, const KwsIO* io, KwsResult* res);
    // offline_greedy_samples' fbank + pad + encoder with the spotter as the stage behind them: encoder_out stays on the device, every
    // stream is searched over all T' frames (io[b].T is not read)
    void kws_samples(const float* const* samples, const int64_t* n_samples, int B, const KwsIO* io, KwsResult* res, int32_t* Tp_out);
    // ---- keyword spotting for CTC models: trie Viterbi on the CTC trellis (ctc_kws.hip; semantics in include/k2hip.h "Keyword spotting
    // for CTC models") ----
    // A graph's tables on the host, each [S]: uploaded with every call (six words per state; there are no decoder rows to keep), the
    // streams of one call that name the same block sharing one copy.  A table block must outlive the call only.
    struct CtcKwsGraph {
        const int32_t *parent, *tok, *depth, *kw;
        const float* bar;
        const int32_t* rc;
        int S;
    };
    // One stream of a chunk call: its graph, the T frames it takes (0: untouched) and its carried block (ctc_kws_ref.h): v / st [2][S]
    struct CtcKwsIO {
        const CtcKwsGraph* graph;
        int T;
        const float* v;
        const int32_t* st;
    };
    // log_probs [B][Tc][V] on the host; the arguments are checked before any device work, and nothing of `io` is written.  The result is
    // a KwsResult whose a / st hold the new blocks, stream b's 2 * S entries at 2 * state_off[b].
    void ctc_kws_chunk_host(const float* log_probs, int B, int Tc, const CtcKwsIO* io, KwsResult* res);
    // offline_greedy_samples' fbank + pad + encoder with the spotter as the stage behind them: the log-probs stay on the device, every
    // stream is searched over all T' frames (io[b].T is not read)
    void ctc_kws_samples(const float* const* samples, const int64_t* n_samples, int B, const CtcKwsIO* io, KwsResult* res, int32_t* Tp_out);
    // ---- CTC prefix beam search with N-best (ctc_prefix.hip; semantics in include/k2hip.h) ----
    // log_probs [R][Tp][V] on the host; n_frames [R] or null (= Tp).  tokens / timestamps / token_log_probs [R][nbest][max_tokens],
    // n_tokens / scores [R][nbest], n_hyps [R]: the shapes of k2hip_beam_search_nbest.  The arguments are checked on the host before
    // any device work (ctc_prefix_ref.h); the engine's decoding method and N-best setting are not affected.
    void ctc_prefix_host(const float* log_probs, int R, int Tp, const int32_t* n_frames, int beam, int nbest, int64_t* tokens, int32_t* timestamps,
                         float* token_log_probs, int32_t* n_tokens, int32_t* n_hyps, float* scores, int max_tokens);
    // decoding method of a CTC model's batch entries: 0 = the reference's argmax-and-collapse, K >= 1 = the prefix beam search with beam K
    // (the single-stream path always collapses)
    // operator level of the resumed prefix search (streaming): log_probs [B, Tc, V] host, n_frames [B] in [1, Tc] or null, in / out
    // blocks of CtcPrefixResumeLayout{K, Tc} (host; the stream histories of ctc_prefix_hist.h fill and apply them).  One upload, one
    // launch, one download; the arguments are checked on the host before any device work.
    void ctc_prefix_chunk_host(const float* log_probs, int B, int Tc, const int32_t* n_frames, int K, const int* in, int* out);
    void set_ctc_prefix(int k) { ctc_prefix_ = k; }
    // Hotword and n-gram LM biasing of the OFFLINE prefix search (k2hip_set_ctc_prefix_biasing; off by default).  On: ctc_prefix_device
    // runs the biased instantiation over the tables of set_hotword_tables / set_ngram_tables when at least one is set; off, or with
    // neither set: the plain instantiation, bit for bit what it always gave.  The carried streaming search never looks at it.
    void set_ctc_prefix_biasing(bool on);
    bool ctc_prefix_biasing() const { return ctc_prefix_biasing_; }
    int ctc_prefix() const { return ctc_prefix_; }
    // ---- fused paths ----
    void offline_greedy_feats(const float* const* feats, const int64_t* n_floats, int B, bool single, int64_t* tokens,
                              int32_t* ts, int32_t* n_tokens, int max_tokens);
    void offline_greedy_samples(const float* const* samples, const int64_t* n_samples, int B, int64_t* tokens,
                                int32_t* ts, int32_t* n_tokens, int max_tokens, bool single = false, bool pinned_src = false);
    void offline_greedy_samples_dev(const float* samples_dev, int64_t n_each, int B, int64_t* tokens, int32_t* ts,
                                    int32_t* n_tokens, int max_tokens);

    // ---- input at another sample rate (resample.hip; DESIGN.md "Input at other sample rates") ----
    // One signal of a resample_host call: outputs k0 .. k0 + n_out of `plan` over the input [head ; tail], whose first float is input
    // sample x0 of its stream, into out (host).  The plans are the caller's (api.cpp keeps them per model and input rate); their tables
    // are uploaded once per input rate and stay resident.
    struct ResampleJob {
        const ResamplePlan* plan;
        const float* head;
        int64_t n_head;
        const float* tail;
        int64_t n_tail;
        int64_t x0, k0, n_out;
        float* out;
    };
    // G signals, any mix of plans, in ONE resample_gather launch: one upload of the staged inputs, one download of the outputs
    void resample_host(const ResampleJob* jobs, int G);
    // Streams of the next from-samples batch that hold input at another rate: entry b names stream b's plan (null: the stream holds
    // samples at the model's rate), the input index x0 of its first queued sample and the outputs k0 it has consumed; its n_samples
    // counts INPUT samples.  While set (the caller clears it after the call), offline_samples counts with the outputs the queued input
    // gives and fills the dense sample block through resample_gather; with no plan in the batch it issues exactly the launches it
    // always did.
    struct WaveSrc {
        const ResamplePlan* plan = nullptr;
        int64_t x0 = 0, k0 = 0;
    };
    void set_wave_srcs(const WaveSrc* w) { wave_srcs_ = w; }

    // ---- voice activity detection and long recordings (vad.hip; the definition: vad_ref.h, DESIGN.md "Voice activity detection and
    // long recordings") ----
    // One stream of a VAD call: its config (checked by the caller: vad_check_config), its carried state (host; replaced by the call),
    // and its input -- n feature rows in `feats` (host), or the samples [head ; tail] (host), whose whole frames are taken: the call
    // sets n to their count.  n == 0 leaves the stream untouched.  The reported segments are appended to *segs.
    struct VadJob {
        const k2hip_vad_config* cfg = nullptr;
        VadState* st = nullptr;
        const float* feats = nullptr;
        int64_t n = 0;
        const float *head = nullptr, *tail = nullptr;
        int64_t n_head = 0, n_tail = 0;
        std::vector<VadSeg>* segs = nullptr;
    };
    // One upload (descriptors, carried blocks, input), the launches of vad_run (behind one batched fbank launch with from_samples: the
    // features never leave the device), one download (new blocks, raw segments, taps).  Everything is checked on the host before any
    // device work; a failed call leaves every state as it was.
    void vad_host(VadJob* jobs, int B, bool from_samples);
    // the taps of the last vad_host call: m, n, d of job b's frames at [off[b], off[b + 1])
    struct VadTaps {
        std::vector<float> m, n;
        std::vector<uint8_t> d;
        std::vector<int64_t> off;
    };
    const VadTaps& last_vad_taps() const { return vad_taps_; }
    // A long recording at the model's rate: fbank over all of it into a resident [T][feat] block, the detector and its flush over the
    // block, the segments packed into batches (vad_pack_batches), each batch gathered device to device into the pad stage and decoded by
    // the model's current search, the best hypothesis kept.  At most kLongMaxSamples samples (K2HIP_ERR_UNSUPPORTED beyond).
    struct LongSegment {
        int64_t start = 0, end = 0;       // frames [start, end) of the recording
        int32_t forced = 0, batch = 0;
        std::vector<int64_t> tokens;
        std::vector<int32_t> timestamps;  // segment-local encoder frames
    };
    static constexpr int64_t kLongMaxSamples = (int64_t)1 << 27;   // 2 h 19 min at 16 kHz: 512 MiB of samples, 256 MiB of features
    void recognize_long(const float* samples, int64_t n, const k2hip_vad_config& cfg, int max_batch, int64_t max_batch_frames,
                        std::vector<LongSegment>* out);
    // legs of the last recognize_long in milliseconds of host time: fbank (with the upload), the detector, the batches
    const std::array<double, 3>& last_long_ms() const { return long_ms_; }

    // ---- neural LM rescoring (rnn_lm.hip; the definition: rnn_lm_ref.h, DESIGN.md "Neural LM rescoring") ----
    // The LM's weights in the layouts the kernels want, ONE device allocation that the caller owns (dev_free), as for the hotword and
    // n-gram tables; *out names its parts.
    void* rnn_lm_upload(const RnnLm& lm, RnnLmDev* out);
    // the LM the scoring entry runs: the caller's host copy (dimensions, sos / eos) and its resident form; null = none
    void set_rnn_lm(const RnnLm* host, const RnnLmDev& dev) { rnn_host_ = host; rnn_dev_ = host ? dev : RnnLmDev{}; }
    bool has_rnn_lm() const { return rnn_host_ != nullptr; }
    // Neural LM shallow fusion (k2hip_set_rnn_lm_fusion): with `on`, an attached LM and scale > 0 the offline modified beam search of
    // the synchronous entries (the ones that keep an N-best list: not the pipelined route, not recognize_long) adds the LM's term
    // during the search; every other path runs as before
    void set_rnn_lm_fusion(bool on, float scale) { rnn_fusion_ = on; rnn_fuse_scale_ = scale; }
    bool rnn_lm_fusion_active() const { return rnn_fusion_ && rnn_host_ && rnn_fuse_scale_ > 0.f && rnn_dev_.w_out; }
    // Neural LM shallow fusion in the STREAMING modified beam search (k2hip_set_rnn_lm_stream_fusion; a switch of its own: the offline
    // one above never reaches a streaming entry).  Active with `on`, an attached LM with its fused layouts and scale > 0.  The caller
    // of a chunk call (k2hip_beam_search_chunk, k2hip_online_step) then names the streams' state blocks (set_beam_nlm_io: a host table
    // of B entries, one per stream of the call in its order; null again after the call): the table is staged with the in blocks, the
    // resumed search takes the per-frame launch form with the LM launches behind every frame, and the blocks' other halves hold the
    // survivors' state afterwards.  Flipping the halves is the caller's, after success.
    void set_rnn_lm_stream_fusion(bool on) { rnn_stream_fusion_ = on; }
    bool rnn_lm_stream_fusion_active() const { return rnn_stream_fusion_ && rnn_host_ && rnn_fuse_scale_ > 0.f && rnn_dev_.w_out; }
    void set_beam_nlm_io(const NlmStreamIO* host) { nlm_io_host_ = host; }
    // the fused search's layouts of the attached LM (rnn_lm_fusion_upload): built when fusion is first switched on, never for a model
    // that only rescores; ONE more device allocation that the caller owns, *io = the attached LM's tables, completed
    void* rnn_lm_fusion_upload(const RnnLm& lm, RnnLmDev* io);
    const RnnLmDev& rnn_lm_dev() const { return rnn_dev_; }
    // k_nlm_advance launches of this model's LM that swept their weights / that only moved state (k2hip_debug.h)
    void rnn_lm_fusion_work(int64_t* swept, int64_t* idle);
    // tuning record: milliseconds per k_nlm_advance launch of `rows` rows that all append, input and hidden width H (a layer above the
    // first: 2 H products per gate), a scattered parent map, pseudo-random operands, `iters` launches between two events
    void nlm_advance_bench(int rows, int H, int iters, float* ms);
    // Hn hypotheses back to back in `tokens` (hypothesis i at [offsets[i], offsets[i + 1])) scored by the attached LM: one upload (ids,
    // targets, descriptors), the launches of the plan (rnn_lm_plan.h), one download.  token_log_probs (may be null) packed per hypothesis
    // in the caller's order, totals [Hn].  Everything is checked on the host before any device work; a call without a position issues
    // none.
    void rnn_lm_score_host(const int64_t* tokens, const int64_t* offsets, int Hn, bool with_eos, float* token_log_probs, float* totals);
    // scoring calls that reached the device since the model was created, and the time blocks of the last one (k2hip_debug.h)
    int64_t rnn_lm_device_calls() const { return rnn_calls_; }
    int rnn_lm_last_blocks() const { return rnn_last_blocks_; }
    // While on, every scoring call brackets its legs with events and waits for them: milliseconds of the last call's embed, GX, steps and
    // score legs (tools/rnn_lm_bench.py)
    void set_rnn_lm_timing(bool on) { rnn_timing_ = on; }
    const std::array<double, 4>& rnn_lm_last_ms() const { return rnn_ms_; }
    // tuning record: milliseconds per recurrent step of `a` rows at hidden width H on pseudo-random operands, `iters` launches timed
    // between two events: the fused step kernel, and the same step composed from the GEMM launcher and lstm_cell (as lstm_layer does)
    void rnn_lm_step_bench(int a, int H, int iters, float* fused_ms, float* composed_ms);

    // ---- pipelined (asynchronous) form of offline_greedy_samples_dev ----
    // submit() enqueues fbank + pad + encoder on the encoder stream and the greedy loop + D2H
    // on a second stream, then returns; wait() blocks on that batch only.  With two batches in
    // flight the latency-bound greedy loop (one or two workgroups per stream) of batch i overlaps the MFMA-bound
    // encoder of batch i+1.  At most kSlots batches may be outstanding.  The third slot is for searches that are LONGER than an
    // encoder pass once they share the GPU with one (modified beam search: 4 launches per frame, each waiting for workgroup slots
    // between the encoder's whole-chip launches): every slot's search then runs on the slot's own stream, so the searches of
    // batches i and i+1 overlap each other and the encoder of batch i+2 (pipe mode 2, automatic with set_beam > 0).
    static constexpr int kSlots = 3;
    int submit_samples_dev(const float* samples_dev, int64_t n_each, int B, int max_tokens);
    int submit_samples_host(const float* samples_host, int64_t n_each, int B, int max_tokens);
    void wait_ticket(int ticket, int64_t* tokens, int32_t* ts, int32_t* n_tokens);

    // ---- streaming (OnlineRecognizer) path: online_engine.cpp ----
    int online_alloc_slot();   // GetEncoderInitStates: a zeroed slot of the device state pool
    void online_free_slot(int slot);
    void online_read_state(int slot, int layer, int kind, long long chunks_done, float* out, int64_t cap, int64_t* n);
    int online_tc50() const;
    int online_frames_per_chunk() const;
    // one tick over B streams that each have a full chunk: chunks [B][T*feat] (host), hyps [B][2], plens [B]
    // nchunks [B]: chunks each stream has decoded before this step (position of its attention rings)
    // chunks: [B] pointers to each stream's T*feat chunk floats (gathered into pinned staging by the engine)
    // operator level (IOnlineProj.EncoderProj): one chunk of the streaming Zipformer2 encoder for B state slots, encoder_out to host
    void online_encoder(const int* slots, const float* feats, const long long* plens, const int* nchunks, int B, float* enc_out);
    // fifo_heads (optional): ring row of every stream's first FIFO frame in the device mirror -- the chunk inputs are then gathered
    // on the device and `chunks` is not read
    void online_step(const int* slots, const float* const* chunks, const long long* hyps, const long long* plens, const int* nchunks, int B,
                     int64_t* tokens, int32_t* ts, int32_t* n_tokens, const int* fifo_heads = nullptr);
    // the same tick under modified beam search with beam K, resumed from each stream's saved hypotheses: beam_in [B] blocks of
    // BeamResumeLayout{K, T'}.in_ints() ints (uploaded with the tick's inputs), beam_out [B] blocks of out_ints() (the tick's one
    // download).  Transducer models only.
    void online_step_beam(const int* slots, const float* const* chunks, const long long* plens, const int* nchunks, int B, int K,
                          const int* beam_in, int* beam_out, const int* fifo_heads = nullptr);
    // the tick of a CTC model under the carried prefix search with beam K: cp_in [B] blocks of CtcPrefixResumeLayout{K, T'}.in_ints() ints
    // (uploaded with the tick's inputs), cp_out [B] blocks of out_ints() (the tick's one download); the resumed kernel runs on the
    // tick's log-probs.  CTC models only.
    void online_step_ctc_prefix(const int* slots, const float* const* chunks, const long long* plens, const int* nchunks, int B, int K,
                                const int* cp_in, int* cp_out, const int* fifo_heads = nullptr);
    // operator level of the resumed search: enc [B, Tp, J] host, in / out blocks of BeamResumeLayout{K, Tp} (host)
    void beam_chunk_host(const float* enc, int B, int Tp, int K, const int* beam_in, int* beam_out);
    // The two entry points above with per-stream hotword graphs (BeamArgs::hw_streams): side blocks of their own beside the
    // BeamResumeLayout blocks, all host memory -- graphs [B] (device tables; all null = that stream is unbiased), st_in [B][K] the
    // graph states of the saved hypotheses, st_out [B][K] those of the survivors.  They ride in the same upload / download.
    struct BeamHwIO {
        const BeamHwStream* graphs;
        const int* st_in;
        int* st_out;
        // the model's n-gram LM runs in this call: st_in / st_out are [2][B][K], the hypotheses' LM states behind their graph states
        bool lm = false;
        // the model's LODR LM runs in this call (only beside an active streaming neural LM fusion): one more [B][K] plane behind those,
        // the hypotheses' LODR states
        bool lodr = false;
        int planes() const { return 1 + (lm ? 1 : 0) + (lodr ? 1 : 0); }
    };
    void online_step_beam_hw(const int* slots, const float* const* chunks, const long long* plens, const int* nchunks, int B, int K,
                             const int* beam_in, int* beam_out, const BeamHwIO& hw, const int* fifo_heads = nullptr);
    void beam_chunk_host_hw(const float* enc, int B, int Tp, int K, const int* beam_in, int* beam_out, const BeamHwIO& hw);
    // The two entry points of the carried CTC prefix search with biasing (ctc_prefix_resume_biased): side blocks of their own beside the
    // CtcPrefixResumeLayout blocks, all host memory -- graphs [B] (device tables; all null = that stream reads no graph), side_in [B]
    // blocks of CtcPrefixResumeBiasLayout{K}.in_ints() ints (flag bit 0: the stream runs the LM), side_out [B] blocks of out_ints().
    // lm: the tables of set_ngram_tables go along (false: null tables, whatever the flags say).  They ride in the same upload / download.
    struct CtcPrefixBiasIO {
        const BeamHwStream* graphs;
        const int* side_in;
        int* side_out;
        bool lm = false;
    };
    void ctc_prefix_chunk_host_bias(const float* log_probs, int B, int Tc, const int32_t* n_frames, int K, const int* in, int* out,
                                    const CtcPrefixBiasIO& bias);
    void online_step_ctc_prefix_bias(const int* slots, const float* const* chunks, const long long* plens, const int* nchunks, int B, int K,
                                     const int* cp_in, int* cp_out, const CtcPrefixBiasIO& bias, const int* fifo_heads = nullptr);

    void set_instrument(bool on) { instrument_ = on; }
    const std::vector<GemmLaunchRec>& gemm_log() const { return gemm_log_; }
    // decoding method of the batch entry points: 0 = greedy_search (the reference's only method), K >= 1 = modified beam
    // search with beam K (BASELINE.json configs[2]); the single-stream path is always greedy
    void set_beam(int k) { beam_ = k; }
    int beam() const { return beam_; }
    const std::vector<int>& last_trail() const { return last_trail_; }
    const std::vector<int>& last_any() const { return last_any_; }
    const std::vector<float>& last_scores() const { return last_scores_; }
    // K2HIP_BEAM_TRACE: [B][Tp][2 beam + 1] words of the last synchronous beam search (BeamArgs::trace), and its B / Tp / beam
    const std::vector<int>& last_beam_trace(int* B, int* Tp, int* K) const {
        *B = last_trace_shape_[0]; *Tp = last_trace_shape_[1]; *K = last_trace_shape_[2];
        return last_beam_trace_;
    }
    const k2hip_timing& timing() const { return timing_; }
    // hotword tables of the offline modified beam search (BeamArgs::hw_*): device memory owned by the caller (api.cpp
    // k2hip_set_hotwords, which allocates, uploads and frees it through dev_alloc / dev_upload / dev_free); null = none
    void set_hotword_tables(const int* next, const float* bonus, const float* pending) {
        hw_next_ = next; hw_bonus_ = bonus; hw_pending_ = pending;
    }
    bool has_hotwords() const { return hw_next_ != nullptr; }
    // n-gram LM of the offline modified beam search (BeamArgs::lm): the scaled tables in device memory owned by the caller (api.cpp
    // k2hip_set_ngram_lm, as for the hotword tables); null tables = none
    void set_ngram_tables(const BeamLm& lm) { lm_ = lm; }
    bool has_ngram_lm() const { return lm_.states != nullptr; }
    // LODR LM (BeamArgs::lodr): the tables scaled by the weight <= 0, device memory owned by the caller (api.cpp k2hip_set_lodr_lm); null
    // tables = none.  Read only by a search the neural LM is fused into; every other search ignores them.
    void set_lodr_tables(const BeamLm& lm) { lodr_ = lm; }
    bool has_lodr_lm() const { return lodr_.states != nullptr; }
    // N-best and token log-probs of the synchronous modified beam search (semantics in include/k2hip.h): 0 = off, nothing is computed
    // or kept beyond the best hypothesis; n >= 1 = every search keeps its first n final hypotheses in pick order, each with its token
    // log-probs, and last_nbest() holds them after the call (entry 0 = the result the call returned)
    struct NbestHost {
        int B = 0, N = 0, max_tokens = 0;
        std::vector<int64_t> tokens;      // [B][N][max_tokens]
        std::vector<int32_t> timestamps;  // [B][N][max_tokens]
        std::vector<float> token_log_probs;
        std::vector<int32_t> n_tokens;    // [B][N]
        std::vector<float> scores;        // [B][N]
        std::vector<int32_t> n_hyps;      // [B]
    };
    // The resumed (streaming) search: while a host buffer is named here, every resumed search also returns the token log-probs of its
    // survivors' suffixes, [B][K][Tp] floats (BeamArgs::yp_out), into it.  The caller names it for one call and clears it.
    void set_beam_yp_out(float* host) { yp_host_ = host; }
    void set_nbest(int n) { nbest_ = n; }
    int nbest() const { return nbest_; }
    const NbestHost& last_nbest() const { return last_nbest_; }
    int batches_in_flight() const {
        int n = 0;
        for (const auto& sl : slots_) n += sl.busy;
        return n;
    }

    float debug_gemm(int M, int N, int K, int act, bool with_res, int iters, int cfg, float* max_err);
    // test hook: ONE launch of configuration `cfg` (-1 = the dispatcher's own choice) on the caller's operands, result back to the host --
    // what tests/test_gemm_gpu.py holds against a float64 product computed on the host (k2hip_debug.h: k2hip_debug_gemm_run)
    void debug_gemm_host(const float* A, const float* W, const float* bias, const float* res, float* C, int M, int N, int K, int act,
                         int glu, int glu_cols, int cfg);
    void debug_gemm_trace(int M, int N, int K, int act, bool with_res, int cfg, unsigned long long* out, int64_t cap, int* n_wg, int* n_waves);
    // test hook: ONE launch of the launcher `op` (kernels.h) on host operands, every buffer uploaded into a NaN-guarded allocation, the
    // guards checked after the launch, the buffers flagged in out_mask downloaded (k2hip_debug.h: k2hip_debug_op_run)
    void debug_op_host(const char* op, const int64_t* iargs, int n_iargs, void* const* bufs, const int64_t* buf_bytes, int n_bufs,
                       uint32_t out_mask);
    // ... reached by api.cpp through this pointer, which engine.cpp sets when the library loads: the host-only builds of api.cpp
    // (tests/native, over a CPU stand-in of the engine) have no kernels to launch, the pointer stays null there and the hook reports
    // K2HIP_ERR_UNSUPPORTED
    using DebugOpFn = void (Engine::*)(const char*, const int64_t*, int, void* const*, const int64_t*, int, uint32_t);
    static inline DebugOpFn debug_op = nullptr;
    void* dev_alloc(int64_t bytes);
    void dev_free(void* p);
    void dev_upload(void* dst, const void* src, int64_t bytes);
    void* host_alloc(int64_t bytes);
    void host_free(void* p);
    void synchronize();

  private:
    // device-side building blocks; all take a Ctx (dry run = sizing only)
    float* encoder_embed(const Ctx& c, const float* x, int B, int T, int* T50);
    // Where a Zipformer2 / Zipformer v1 stack walk and its layers run.  A null site is offline: whole utterances.  Otherwise one chunk of
    // the streams in these state slots (device arrays of B entries each), behind the config's per-stack left context.
    struct StreamSite {
        const int* d_slots;
        const long long* d_plen = nullptr;   // frames each stream has processed (Zipformer2)
        const int* d_chunks = nullptr;       // chunks each stream has decoded: the position of its rings (Zipformer2)
    };
    // Zipformer2: one layer, the walk over the stacks and the head behind it, offline and streaming (engine.cpp).  gl = global layer index
    void encoder_layer(const Ctx& c, int si, int li, int gl, float* x, const float* pe, int B, int T, const StreamSite* site,
                       const LayerTail* tail = nullptr);
    // true: ended in an offline tap (*tap_ptr, *tap_dim); false: *segs = the pieces of the full-width output
    bool encoder_stacks(const Ctx& c, float* x0, int B, int T50, const StreamSite* site, int tap, float** tap_ptr, int* tap_dim, FullDimSegs* segs);
    // downsample_output + joiner.encoder_proj (CTC: the log_probs head) into enc_out; null: taken from the arena here, last
    float* encoder_head(const Ctx& c, const FullDimSegs& segs, int B, int T50, float* enc_out);
    float* encoder_forward(const Ctx& c, const float* x, int B, int T, int* Tp, int tap, float** tap_ptr, int* tap_rows,
                           int* tap_dim);
    // device by-products of ONE search, in the arena that search ran in: they travel from the search to the finish_tokens of the same
    // call and are kept nowhere else (null = that search has none)
    struct SearchExtras {
        float* scores = nullptr;              // beam: [B] final scores
        BeamNbest nb;                         // beam with N-best kept
        int* trace = nullptr;                 // K2HIP_BEAM_TRACE: [B][Tp][2 K + 1]
        int trace_B = 0, trace_Tp = 0, trace_K = 0;
        int *trail = nullptr, *any = nullptr; // CTC: [B] each
        float* align_lp = nullptr;            // align: [B][max_tokens] token log-probs of the best path
        float* align_scores = nullptr;        // align: [B][2] = (total, best)
        int* align_end = nullptr;             // CTC align: [H][max_tokens] last frame of every token on the best path
        int* kws_start = nullptr;             // keyword spotting: [B][max_tokens] start frames, sum_logp, and the new carried blocks
        float* kws_sum = nullptr;
        float* kws_a = nullptr;
        int* kws_st = nullptr;
        int kws_states = 0;
    };
    // One keyword-spotting call as the host lays it out before any device work: the streams' descriptors and carried blocks in ONE upload
    struct KwsPlan {
        int B = 0, Tp = 0, max_T = 0, max_S = 0, n_states = 0;
        long long plane_floats = 0;
        int64_t o_a = 0, o_st = 0;        // byte offsets of the carried values (float) and starts (int) behind the descriptors
        std::vector<int32_t> state_off;
        std::vector<char> blob;
    };
    KwsPlan kws_plan(int B, int Tp, const KwsIO* io, bool all_frames) const;
    // trie_logprobs, trie_dp into `out` (tokens = keywords, timestamps = end frames, counts = events).  The test hooks pass planes of
    // their own (stay / emit) and stop after the first kernel (dp = false) or run only the second (cells = false).
    SearchExtras kws_device(const Ctx& c, const float* enc, int Tp, const KwsPlan& p, const SearchOut& out, float* stay = nullptr,
                            float* emit = nullptr, bool cells = true, bool dp = true);
    // a finished call's results (the SearchOut rows of mt entries and the last_kws_* vectors) into `res`; state_off is the plan's, either spotter's
    void kws_collect(const std::vector<int32_t>& state_off, int mt, std::vector<int64_t>&& tok, std::vector<int32_t>&& ts, std::vector<int32_t>&& n, KwsResult* res) const;
    std::vector<int32_t> last_kws_start_, last_kws_st_;
    std::vector<float> last_kws_sum_, last_kws_a_;
    // One CTC keyword-spotting call as the host lays it out before any device work: the streams' descriptors, carried blocks and the
    // distinct graphs' tables in ONE upload
    struct CtcKwsPlan {
        int B = 0, Tp = 0, V = 0, max_T = 0, max_S = 0, n_states = 0;
        int64_t o_v = 0, o_st = 0, o_tab = 0;   // byte offsets of the carried values, starts and the tables behind the descriptors
        std::vector<int32_t> state_off;
        std::vector<char> blob;
    };
    // V: the width of the log-probs, 0 = the model's vocabulary (the test hook passes planes of any width)
    CtcKwsPlan ctc_kws_plan(int B, int Tp, const CtcKwsIO* io, bool all_frames, int V = 0) const;
    // ctc_trie_dp into `out` (tokens = keywords, timestamps = end frames, counts = events); the new blocks and the events' starts and
    // sums travel in the kws_* extras
    SearchExtras ctc_kws_device(const Ctx& c, const float* logp, int Tp, const CtcKwsPlan& p, const SearchOut& out);
    // One align call as the host lays it out before any device work: the streams' descriptors, targets and contexts in ONE upload block
    struct AlignPlan {
        int B = 0, Tp = 0, max_T = 0, max_U = 0, n_ctx = 0, n_ids = 0;
        long long plane_floats = 0, bp_words = 0;
        int64_t o_ids = 0, o_ctx = 0;     // byte offsets of the targets (int) and the contexts (long long [n_ctx][2]) behind the descriptors
        std::vector<char> blob;
        const AlignStream* streams() const { return reinterpret_cast<const AlignStream*>(blob.data()); }
    };
    AlignPlan align_plan(int B, int Tp, const int32_t* n_frames, const int64_t* ids, const int32_t* lens, int max_tokens) const;
    // decoder over every context, lattice_logprobs, lattice_dp into `out` (tokens = the targets, counts = their lengths).  The test hooks
    // pass planes of their own (stay / emit) and stop after the first kernel (dp = false) or run only the second (cells = false).
    SearchExtras align_device(const Ctx& c, const float* enc, int Tp, const AlignPlan& p, const SearchOut& out, float* stay = nullptr,
                              float* emit = nullptr, bool cells = true, bool dp = true);
    std::vector<float> last_align_lp_, last_align_scores_;
    // One CTC align call as the host lays it out before any device work: the targets' descriptors and ids (stream_of resolved into
    // CtcAlignTarget::row) in ONE upload block
    struct CtcAlignPlan {
        int R = 0, Tp = 0, H = 0, max_T = 0, max_U = 0, n_ids = 0;
        long long plane_floats = 0, bp_words = 0;
        int64_t o_ids = 0;                // byte offset of the targets (int) behind the descriptors
        std::vector<char> blob;
        const CtcAlignTarget* targets() const { return reinterpret_cast<const CtcAlignTarget*>(blob.data()); }
    };
    CtcAlignPlan ctc_align_plan(int R, int Tp, const int32_t* n_frames, int H, const int32_t* stream_of, const int64_t* ids, const int32_t* lens,
                                int max_tokens) const;
    // gather + lattice into `out` (H rows: tokens = the targets, counts = their lengths, timestamps); end frames, token log-probs and
    // (total, best) are SearchExtras
    SearchExtras ctc_align_device(const Ctx& c, const float* logp, int R, int Tp, const CtcAlignPlan& p, const SearchOut& out);
    std::vector<int32_t> last_align_end_;
    // what an align call has finish_tokens fill (only the timestamps are read back): rows of mt = max(max_tokens, 1) entries
    struct AlignScratch {
        int mt;
        std::vector<int64_t> tok;
        std::vector<int32_t> ts, n;
        AlignScratch(int rows, int max_tokens) : mt(std::max(max_tokens, 1)), tok((size_t)rows * mt), ts((size_t)rows * mt), n((size_t)rows) {}
    };
    // lens[r] entries of row r from the scratch and the last_align_* vectors into the caller's outputs (each may be null)
    void align_copy_out(int rows, const int32_t* lens, const AlignScratch& s, int32_t* timestamps, int32_t* end_frames, float* token_log_probs,
                        float* total, float* best) const;
    // What a call runs on the encoder output, named by the caller: one plan's alignment, or (both null) the model's search.
    // keep_nbest: the caller fetches the beam search's N-best (the synchronous entries; the pipelined route has no place to keep them)
    struct SearchStage {
        bool single = false, keep_nbest = true;
        const AlignPlan* align = nullptr;
        const CtcAlignPlan* ctc_align = nullptr;
        const KwsPlan* kws = nullptr;
        const CtcKwsPlan* ctc_kws = nullptr;
        // rows of its search-output block for B streams: one per stream, or one per target (several CTC targets may share a stream)
        int rows(int B) const { return ctc_align ? ctc_align->H : B; }
    };
    SearchExtras search_device(const Ctx& c, const float* enc, int B, int Tp, const SearchStage& stage, const SearchOut& out);
    // the model's search alone: CTC collapse, modified beam search or greedy
    SearchExtras greedy_device(const Ctx& c, const float* enc, int B, int Tp, bool single, const SearchOut& out, bool keep_nbest);
    // the operator entries' route: host encoder_out (a CTC model's log_probs) uploaded, the stage run on it, the results fetched
    void search_host(const float* enc_out, int B, int Tp, const SearchStage& stage, int64_t* tokens, int32_t* ts, int32_t* n_tokens, int max_tokens);
    // the fused offline entries' tail on c.stream: event 2, encoder, event 3, the stage, event 4
    SearchExtras encode_and_search(const Ctx& c, const float* d_x, int B, int T, const SearchStage& stage, const SearchOut& out);
    // One offline batch's shape from its longest stream (samples, or feature floats with from_feats): its feature frames and floats, the
    // padded length L in floats, the encoder's input frames T and output frames Tp
    struct OfflineShape {
        int64_t longest, frames, n_fl, L;
        int T, Tp;
    };
    OfflineShape offline_shape(const char* who, int64_t longest, bool from_feats = false) const;
    // ... of host sample arrays of any lengths, each of which must give a frame
    OfflineShape samples_shape(const float* const* samples, const int64_t* n_samples, int B) const;
    // T' of that batch, over all of which the fused align / keyword entry `who` runs its search; a batch that gives no encoder frame is refused
    int samples_frames(const char* who, const float* const* samples, const int64_t* n_samples, int B) const;
    // fbank's arguments, the model's constants filled in
    FbankArgs fbank_args(const float* src, int64_t n, int64_t stride, int n_utts, int64_t nf, float* dst) const;
    // offline_greedy_samples with the stage named: what the public entry and the two align entries run
    void offline_samples(const float* const* samples, const int64_t* n_samples, int B, const SearchStage& stage, int64_t* tokens, int32_t* ts,
                         int32_t* n_tokens, int max_tokens, bool pinned_src);
    const WaveSrc* wave_srcs_ = nullptr;
    // the core of vad_host / recognize_long: jobs whose feature rows are on the device (d_feats[b], rows `feat` floats apart; filled in by
    // `prepare`, which runs inside the sized body in front of the detector and enqueues whatever produces the rows)
    void vad_device_call(VadJob* jobs, int B, const std::function<void(const Ctx&, std::vector<const float*>&)>& prepare);
    VadTaps vad_taps_;
    std::array<double, 3> long_ms_{};
    const RnnLm* rnn_host_ = nullptr;
    RnnLmDev rnn_dev_;
    bool rnn_fusion_ = false;
    bool rnn_stream_fusion_ = false;
    const NlmStreamIO* nlm_io_host_ = nullptr;
    float rnn_fuse_scale_ = 0.f;
    int64_t rnn_calls_ = 0;
    int rnn_last_blocks_ = 0;
    bool rnn_timing_ = false;
    std::array<double, 4> rnn_ms_{};
    // samples of the model's rate that stream b of a from-samples batch gives
    int64_t wave_count(int b, int64_t n_samples) const {
        const WaveSrc* w = wave_srcs_ ? wave_srcs_ + b : nullptr;
        return w && w->plan ? w->plan->num_out(w->x0 + n_samples) - w->k0 : n_samples;
    }
    // a plan's tables on the device: one allocation [w | first | ntaps] per input rate, made on first use
    struct ResampleDev {
        char* base = nullptr;
        const float* w = nullptr;
        const int *first = nullptr, *ntaps = nullptr;
    };
    std::map<int, ResampleDev> rs_cache_;
    const ResampleDev& resample_dev(const ResamplePlan& p);
    // the launcher's row for outputs k0 .. k0 + n_out of `p` (null: pass-through) over [head ; tail]
    ResampleRow resample_row(const ResamplePlan* p, const float* head, int64_t n_head, const float* tail, int64_t n_tail, int64_t x0, int64_t k0,
                             int64_t n_out, int dst_row);
    // timing_ from ev_[0..5]; which of the legs in front of the encoder the call has
    void fill_timing(bool fbank_leg, bool pad_leg);
    const float* pos_emb(int T);  // cached CompactRelPositionalEncoding table on device
    // linear_pos(pos_emb) of one layer: [rows, ncols] = pe [rows, pe_dim] . W^T.  It does not depend on the audio, so it is computed
    // once per (layer, rows) and kept on the device (a handful of utterance lengths in flight; the cache is dropped when it grows)
    const float* pos_proj_cached(const Ctx& c, int layer, const float* pe, int pe_dim, const float* W, int rows, int ncols);
    std::map<std::pair<int, int>, float*> pp_cache_;
    size_t pp_cache_bytes_ = 0;
    SearchExtras ctc_device(const Ctx& c, const float* logp, int B, int Tp, const SearchOut& out);
    SearchExtras beam_device(const Ctx& c, const float* enc, int B, int Tp, const SearchOut& out, bool keep_nbest);
    // the prefix beam search over logp [R][Tp][V] (device; V is the call's): the best hypothesis into `out`, scores in ex.scores, and --
    // with keep_nbest and set_nbest(n > 0) -- the first n slots in ex.nb.  n_frames: host [R] or null.
    SearchExtras ctc_prefix_device(const Ctx& c, const float* logp, int R, int Tp, int V, const int32_t* n_frames, int beam, const SearchOut& out,
                                   bool keep_nbest);
    // hw (device pointers) or null: the unbiased search, today's launch
    void beam_resume_device(const Ctx& c, const float* enc, int B, int Tp, int K, const int* d_in, int* d_out, int* d_overflow,
                            const BeamHwIO* hw = nullptr, const NlmStreamIO* d_nlm = nullptr);
    void beam_chunk_impl(const float* enc, int B, int Tp, int K, const int* beam_in, int* beam_out, const BeamHwIO* hw);
    struct OnlineBeamIO { int K; const int* in; int* out; const BeamHwIO* hw; };
    struct OnlineCtcPrefixIO { int K; const int* in; int* out; const CtcPrefixBiasIO* bias = nullptr; };
    void ctc_prefix_chunk_impl(const float* log_probs, int B, int Tc, const int32_t* n_frames, int K, const int* in, int* out, const CtcPrefixBiasIO* bias);
    void online_step_impl(const int* slots, const float* const* chunks, const long long* hyps, const long long* plens, const int* nchunks,
                          int B, int64_t* tokens, int32_t* ts, int32_t* n_tokens, const int* fifo_heads, const OnlineBeamIO* beam,
                          const OnlineCtcPrefixIO* cpx = nullptr);
    // LSTM transducer (lstm_engine.cpp)
    int lstm_out_frames(int T) const;
    float* lstm_embed(const Ctx& c, const float* x, int B, int T, int* T_out);
    void lstm_layer(const Ctx& c, int li, float* x, const float* h0, int ldh0, float* cst, int B, int T, float* y);
    float* lstm_forward_seq(const Ctx& c, float* xe, int B, int T3, float* enc_out, int tap, float** tap_ptr, int* tap_dim);
    float* lstm_forward(const Ctx& c, const float* x, int B, int T, int* Tp, int tap, float** tap_ptr, int* tap_rows, int* tap_dim);
    float* lstm_chunk(const Ctx& c, const float* x, const int* d_slots, int B);
    // Zipformer v1 (zipformer1_engine.cpp)
    const float* sinus_pos_emb(int Tc, int left, int D);
    std::map<std::tuple<int, int, int>, float*> sinus_cache_;  // (frames, left context, width) -> device table
    float* zip1_embed(const Ctx& c, const float* x, int B, int T, int* Tc_out);
    // one layer and the walk over the stacks (through joiner.encoder_proj), offline (null site) and streaming
    void zip1_layer(const Ctx& c, int si, const std::string& pfx, int l, float* x, const float* pe, int B, int T, const StreamSite* site);
    float* zip1_stacks(const Ctx& c, float* x0, int B, int Tc, const StreamSite* site, float* enc, int tap, float** tap_ptr, int* tap_dim);
    float* zip1_chunk(const Ctx& c, const float* x, const int* d_slots, int B, int* Tp_out);
    float* zip1_forward(const Ctx& c, const float* x, int B, int T, int* Tp, int tap, float** tap_ptr, int* tap_rows, int* tap_dim);
    // offline Conformer (conformer_engine.cpp)
    const float* conformer_pos_emb_left(int Tc, int left);
    float* conformer_chunk(const Ctx& c, const float* x, const int* d_slots, const long long* d_plen, int B, int* Tc_out);
    int conformer_out_frames(int T) const;
    const float* conformer_pos_emb(int T);
    float* conformer_embed(const Ctx& c, const float* x, int B, int T, int* T_out);
    void conformer_layer(const Ctx& c, int li, float* x, const float* pe, int B, int T);
    float* conformer_forward(const Ctx& c, const float* x, int B, int T, int* Tp, int tap, float** tap_ptr, int* tap_rows,
                             int* tap_dim);
    const float* pos_emb_stream(int Tc, int L);
    void online_ensure_pool();
    float* encoder_embed_stream(const Ctx& c, const float* x, const int* d_slots, int B, int T, int* Tc);
    std::mutex cache_mu_;  // pos_proj / pos_emb / decjoin tables are built lazily
    float* online_encoder_zip2(const Ctx& c, const float* d_x, const int* d_slots, const long long* d_plen, const int* d_chunks, int B);
    DecJoinW decjoin();
    float* d_dec_table_ = nullptr;  // [(V + 1) V][J] decoder output of every context (small vocabularies), built on first use
    bool dec_table_tried_ = false;
    float* d_ptab_ = nullptr;  // [2][V][DD] per-token decoder-conv table (groups = 1 models), built on first use

    // run `body` once dry to size the arena, then for real
    template <typename F>
    void run_sized(F&& body);
    int submit_impl(const float* samples_dev, const float* samples_host, int64_t n_each, int B, int max_tokens);
    // The end of every search.  download_search enqueues the block's ONE copy into `pin` on the search's stream; once that copy has
    // landed, settle_search reads the flag, feeds the back-off, repeats a timed-out parted search (`rec`, if it is this block's) with one
    // part per stream and downloads again, and turns what the flag then says into the call's error.
    void download_search(const SearchOut& out, hipStream_t s, void* pin);
    void settle_search(const SearchOut& out, hipStream_t s, GreedyLaunch& rec, void* pin);
    void finish_tokens(const SearchOut& out, const SearchExtras& ex, int64_t* tokens, int32_t* ts, int32_t* n_tokens);
    Ctx make_ctx(bool dry);

    std::unique_ptr<Model> model_;
    int device_;
    hipStream_t stream_ = nullptr;
    Arena arena_;
    Arena* cur_arena_ = &arena_;
    struct Slot {
        Arena arena;
        hipEvent_t enc_done = nullptr, done = nullptr, h2d_done = nullptr;
        hipStream_t stream = nullptr;  // pipe mode 1: the slot's whole pipeline (fbank .. search .. D2H) runs here
        void* pin = nullptr;
        int64_t pin_cap = 0;
        SearchOut out;                  // the batch's token block in `arena`
        int B = 0, max_tokens = 0;      // the batch's shape (all that the CPU stand-ins of the engine under tests/native keep of it)
        bool busy = false;
        GreedyLaunch greedy;            // the slot's search launch, kept for the one-part retry
        hipStream_t search_stream = nullptr;
    } slots_[kSlots];
    GreedyLaunch last_greedy_;          // the same for the synchronous entries (searches on stream_)
    void note_search(bool parted, bool timed_out);
    int one_part_left_ = 0, one_part_span_ = 0;   // searches still to run with one workgroup per stream / the current back-off span
    // [2] rounds of the large-vocabulary search decided by the f16 screen / run by the f32 passes since the model was created, counted
    // only while K2HIP_SCREEN_COUNT is on (k2hip_debug_op_run "greedy_screen_counts")
    unsigned long long* d_screen_counts_ = nullptr;
    unsigned long long* screen_counts() const { return tunables().screen_count ? d_screen_counts_ : nullptr; }
    int search_retries_ = 0;            // one-part retries since the model was created (k2hip_debug_search_retries)
    int next_slot_ = 0;
    hipStream_t stream2_ = nullptr;
    // submit/wait overlap: 0 = search of batch i (stream2) under the encoder of batch i+1 (stream); 1 = every slot owns a
    // stream, so whole batches run concurrently and each other's GEMM prologues / epilogues / tails are filled; 2 = encoders in
    // order on `stream`, every slot's search on the slot's stream (chosen by itself for the beam search)
    float* online_pool_ = nullptr;
    float* online_fifo_ = nullptr;  // [online_cap_][kFifoFrames][feat]
    int online_cap_ = 0;
    std::vector<int> free_slots_;
    OnlineLayout lay_;
    std::mutex mu_;
    std::map<int, float*> pe_cache_;
    bool instrument_ = false;
    int beam_ = 0;
    int ctc_prefix_ = 0;
    bool ctc_prefix_biasing_ = false;
    int nbest_ = 0;
    float *yp_host_ = nullptr, *d_yp_ = nullptr;
    size_t yp_floats_ = 0;
    void fetch_beam_yp();   // after the resumed search's download: d_yp_ -> yp_host_
    NbestHost last_nbest_;
    const int* hw_next_ = nullptr;
    const float *hw_bonus_ = nullptr, *hw_pending_ = nullptr;
    BeamLm lm_;
    BeamLm lodr_;
    // CTC search by-products of the last synchronous call (NumTrailingBlank bookkeeping, OfflineRecognizer.cs:392-397)
    std::vector<int> last_trail_, last_any_;
    std::vector<int> last_beam_trace_;
    int last_trace_shape_[3] = {0, 0, 0};   // its B / Tp / beam
    float* d_dec_start_ = nullptr;  // [2][J]: decoder outputs of the start contexts [-1, blank], [blank, blank] (model constants)
    const float* decoder_start(const Ctx& c);
    std::vector<float> last_scores_;
    GemmStats stats_;
    k2hip_timing timing_{};
    hipEvent_t ev_[8] = {nullptr};
    std::vector<hipEvent_t> evpool_;
    std::vector<GemmLaunchRec> gemm_log_;
    int evused_ = 0;
    // pinned staging for results
    void* pin_ = nullptr;
    int64_t pin_cap_ = 0;
    void* pinned(int64_t bytes);
    void* pin_in_ = nullptr;   // pinned staging of a step's inputs (chunks), separate from the result staging above
    int64_t pin_in_cap_ = 0;
    void* pinned_in(int64_t bytes);
    void* pin_fb_ = nullptr;   // pinned staging of a deferred fbank gather (its frames are collected after the step that follows)
    int64_t pin_fb_cap_ = 0;
    void* pinned_fb(int64_t bytes);
    struct PendingFeats {
        bool active = false;
        std::vector<float*> dst;
        const char* src = nullptr;
        size_t per_out = 0;
    } fb_pending_;
};

// What every C-ABI entry holds while it works on a model: the model's mutex (calls on one handle are serialised) AND the model's
// device made current on the calling thread -- BEFORE anything is created lazily (slot streams, pinned staging, pool growth), so a
// host thread whose current device is another GPU (the C# "8 handles from 8 pool threads" story, IOnlineProj.cs:65-71 /
// SURVEY 8b "hipSetDevice per call") can never place a stream or a buffer on the wrong card.
class EngineLock {
  public:
    explicit EngineLock(Engine& e) : lk_(e.mutex()) { K2_HIP(hipSetDevice(e.device())); }

  private:
    std::lock_guard<std::mutex> lk_;
};

template <typename F>
void Engine::run_sized(F&& body) {
    K2_HIP(hipSetDevice(device_));
    stats_ = GemmStats();
    cur_arena_->reset();
    cur_arena_->set_dry(true);
    try {
        Ctx d = make_ctx(true);
        body(d);
    } catch (...) {
        cur_arena_->set_dry(false);
        cur_arena_->reset();
        throw;
    }
    cur_arena_->set_dry(false);
    int64_t need = cur_arena_->high_water();
    cur_arena_->reset();
    if (need > cur_arena_->capacity()) {
        K2_HIP(hipStreamSynchronize(stream_));
        cur_arena_->reserve(need + need / 8);
    }
    Ctx c = make_ctx(false);
    evused_ = 0;
    gemm_log_.clear();
    body(c);
    if (instrument_) {
        K2_HIP(hipStreamSynchronize(stream_));
        for (int i = 0; i + 1 < evused_; i += 2) {
            float ms = 0;
            K2_HIP(hipEventElapsedTime(&ms, evpool_[i], evpool_[i + 1]));
            stats_.ms += ms;
            if ((size_t)(i / 2) < gemm_log_.size()) gemm_log_[i / 2].us = ms * 1e3f;
        }
    }
    timing_.gemm_ms = stats_.ms;
    timing_.gemm_launches = stats_.launches;
    timing_.gemm_flops = stats_.flops;
    timing_.total_flops = stats_.total_flops;
}


}  // namespace k2hip
