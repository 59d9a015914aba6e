// C ABI of libk2hip.so (include/k2hip.h) + the host-side mirror of the reference's
// OfflineStream / OfflineRecognizer bookkeeping (K2TransducerAsr/OfflineStream.cs,
// OfflineRecognizer.cs:77-91,289-296).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <fstream>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <new>

#include "text.h"
#include "engine.h"
#include "beam_hist.h"
#include "ctc_prefix_hist.h"
#include "hotwords.h"
#include "keywords.h"
#include "kws_ref.h"
#include "resample_ref.h"
#include "ctc_kws_ref.h"
#include "ngram_lm.h"
#include "lodr_host.h"
#include "../../include/k2hip_debug.h"

using namespace k2hip;

// The sample queue of an OfflineStream: a float array in PINNED host memory (Engine::host_alloc), which the GPU reads in place -- the
// batch's GetResults gathers the streams' samples straight out of these buffers (no staging copy on the host, no separate upload).
struct PinVec {
    Engine* e = nullptr;
    float* p = nullptr;
    size_t n = 0, cap = 0;
    PinVec() = default;
    PinVec(const PinVec&) = delete;
    PinVec& operator=(const PinVec&) = delete;
    PinVec(PinVec&& o) noexcept : e(o.e), p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = o.cap = 0; }
    PinVec& operator=(PinVec&& o) noexcept {
        if (this != &o) {
            release();
            e = o.e; p = o.p; n = o.n; cap = o.cap;
            o.p = nullptr; o.n = o.cap = 0;
        }
        return *this;
    }
    ~PinVec() { release(); }
    void release() noexcept {
        if (p && e) {
            try { e->host_free(p); } catch (...) {}
        }
        p = nullptr;
        n = cap = 0;
    }
    const float* data() const { return p; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    size_t capacity() const { return cap; }
    void clear() { n = 0; }
    void append(Engine& eng, const float* src, size_t cnt) {
        if (n + cnt > cap) {   // (a stream normally gets ONE AddSamples call, and its buffer comes from the pool: growth is the rare path)
            const size_t want = std::max(n + cnt, cap + cap / 2);
            const size_t ncap = (want + 65535) & ~(size_t)65535;
            float* q = static_cast<float*>(eng.host_alloc((int64_t)(ncap * sizeof(float))));
            if (n) memcpy(q, p, n * sizeof(float));
            float* old = p;
            e = &eng; p = q; cap = ncap;
            if (old) {
                try { eng.host_free(old); } catch (...) {}   // (the queue is consistent either way)
            }
        }
        memcpy(p + n, src, cnt * sizeof(float));
        n += cnt;
    }
    void erase_front(size_t cnt) {
        if (cnt >= n) { n = 0; return; }
        memmove(p, p + cnt, (n - cnt) * sizeof(float));
        n -= cnt;
    }
};

// A hotword graph resident on a model's device for the streams that attached it (k2hip_online_stream_set_hotwords,
// k2hip_beam_stream_set_hotwords): the dense tables in ONE allocation [next | bonus | pending] and a host copy of pending.  Streams
// hold it through a shared_ptr; the model's cache (k2hip_model::hw_cache, keyed by the graph's serial number) holds a weak one, so
// the tables are freed when the last stream lets go -- or with the model, which then clears `owner` and `dev`: a stream that outlives
// its model drops its reference without touching the model.  g_hw_mu guards the caches, `owner` and `dev` of every model; it is taken
// before an engine lock, never inside one.
struct HwResident {
    uint64_t serial = 0;
    k2hip_model* owner = nullptr;
    void* dev = nullptr;
    BeamHwStream tables;
    std::shared_ptr<const std::vector<float>> pending;
};
// A keyword graph resident on a model's device for the keyword streams created on it (k2hip_kws_stream_create): the decoder rows of
// the trie's contexts and its tables in ONE allocation, shared by the streams of that (model, graph) and released the way HwResident is.
// It also holds the graph itself: a stream outlives the handle it was created from.
struct KwResident {
    uint64_t serial = 0;
    k2hip_model* owner = nullptr;
    void* dev = nullptr;
    KwsGraphDev tables;
    std::shared_ptr<const KeywordGraph> graph;
};
static std::mutex g_hw_mu;
static std::atomic<uint64_t> g_hw_serial{0};

struct k2hip_model {
    Engine engine;
    // Sample buffers of destroyed OfflineStreams, handed to the next streams (a GetResults batch is B x create / AddSamples / destroy
    // of ~640 KB each: pinned allocations cost a system call and a page-table update each, and fresh pages a first-touch fault per 4 KB
    // -- ~1 ms per 32 x 10 s batch on the host thread that drives the GPU).  At most kPoolMax buffers are kept.
    static constexpr size_t kPoolMax = 128;
    std::mutex wav_mu;
    std::vector<PinVec> wav_pool;   // (declared behind `engine`: released first)
    // the hotword tables on the device (k2hip_set_hotwords): one allocation [next | bonus | pending], or null
    void* hw_dev = nullptr;
    // the scaled n-gram LM tables on the device (k2hip_set_ngram_lm): one allocation, or null
    void* lm_dev = nullptr;
    // identity of the LM that is set (0 = none; a fresh number for every k2hip_set_ngram_lm that leaves one set) and its start state:
    // what a stream notes with its first chunk (BeamHistory::begin_lm).  Written and read under the engine's lock.
    uint64_t lm_serial = 0;
    int lm_start = 0;
    int lm_states = 0;   // its number of states (0 = none): what a carried LM state is checked against before a launch
    // LODR (k2hip_set_lodr_lm): the model's own copy of the low-order LM, its scaled automaton on the host (the rescoring walks it) and
    // on the device (the fused searches walk it), and the setting's serial number (0 = none; fresh for every call that leaves one set).
    // Under the engine's lock.
    std::unique_ptr<NgramLm> lodr_lm;
    std::shared_ptr<const LodrHost> lodr_host;
    void* lodr_dev = nullptr;
    uint64_t lodr_serial = 0;
    // the neural LM of k2hip_set_rnn_lm: the model's own host copy (shared with the handle it came from: it is immutable), its weights
    // on the device in one allocation, and the scale of the rescoring (0 = the N-best lists are left alone)
    std::shared_ptr<const RnnLm> rnn_lm;
    void* rnn_dev = nullptr;
    void* rnn_fuse_dev = nullptr;   // the fused search's layouts of the same LM: made when fusion is on, null otherwise
    float rnn_scale = 0.f;
    bool rnn_fusion = false;   // k2hip_set_rnn_lm_fusion: the LM's term is added during the offline modified beam search instead
    // k2hip_set_rnn_lm_stream_fusion: ... and during the streaming one, the hypotheses' LM state carried from chunk to chunk in device
    // blocks of nlm_pool (rnn_lm_stream_pool.h; made on first use, shared with the streams that hold a block, emptied with the model).
    // rnn_serial numbers the settings of k2hip_set_rnn_lm: what a fused stream notes with its first chunk.  Under the engine's lock.
    bool rnn_stream_fusion = false;
    uint64_t rnn_serial = 0;
    std::shared_ptr<NlmStreamPool> nlm_pool;
    // k2hip_set_nbest: 1 = off (the engine keeps nothing beyond the best hypothesis), n > 1 = alternatives and token log-probs are kept
    std::atomic<int> nbest{1};
    // the graphs attached to this model's streams (HwResident), by serial number; hw_uploads counts the uploads (k2hip_debug.h)
    std::map<uint64_t, std::weak_ptr<HwResident>> hw_cache;
    int hw_uploads = 0;
    // the keyword graphs resident for this model's keyword streams (KwResident), by serial number
    std::map<uint64_t, std::weak_ptr<KwResident>> kw_cache;
    // the resampler's plans by input rate (resample_plan.h), built on first use and kept for the model's life: streams and the engine's
    // device tables name them by address
    std::mutex rs_mu;
    std::map<int, std::unique_ptr<ResamplePlan>> rs_plans;
    k2hip_model(const char* path, const char* ov, int dev) : engine(path, ov, dev) {}
    ~k2hip_model() {
        {
            std::lock_guard<std::mutex> g(g_hw_mu);
            for (auto& kv : hw_cache)
                if (auto r = kv.second.lock()) {   // streams still hold it: the tables go with the model, the host part stays theirs
                    try {
                        engine.synchronize();
                        engine.dev_free(r->dev);
                    } catch (...) {
                    }
                    r->dev = nullptr;
                    r->owner = nullptr;
                    r->tables = BeamHwStream{};
                }
            hw_cache.clear();
            for (auto& kv : kw_cache)
                if (auto r = kv.second.lock()) {
                    try {
                        engine.synchronize();
                        engine.dev_free(r->dev);
                    } catch (...) {
                    }
                    r->dev = nullptr;
                    r->owner = nullptr;
                    r->tables = KwsGraphDev{};
                }
            kw_cache.clear();
        }
        if (hw_dev) {
            try {
                engine.synchronize();
                engine.dev_free(hw_dev);
            } catch (...) {
            }
        }
        if (lm_dev) {
            try {
                engine.synchronize();
                engine.dev_free(lm_dev);
            } catch (...) {
            }
        }
        if (lodr_dev) {
            try {
                engine.synchronize();
                engine.dev_free(lodr_dev);
            } catch (...) {
            }
        }
        if (nlm_pool) {   // (streams that still hold a block only forget it from now on)
            try {
                engine.synchronize();
            } catch (...) {
            }
            nlm_pool->shutdown();
        }
        if (rnn_dev || rnn_fuse_dev) {
            try {
                engine.synchronize();
                if (rnn_dev) engine.dev_free(rnn_dev);
                if (rnn_fuse_dev) engine.dev_free(rnn_fuse_dev);
            } catch (...) {
            }
        }
    }
};

// Streaming neural LM shallow fusion: what a stream under the modified beam search notes with its first chunk (whether fusion was
// active, and then the LM's serial and the scale) and the device block that carries its hypotheses' LM state between chunks
struct NlmCarry {
    bool active = false;
    uint64_t serial = 0;
    float scale = 0.f;
    NlmStreamPool::Handle block;
};
// One chunk call's view of the setting (read under the engine's lock), the rule "a stream keeps the setting of its first chunk", the
// block table of the call and the flip after success
struct NlmStreamCall {
    bool active = false;
    uint64_t serial = 0;
    float scale = 0.f;
    int L = 0, H = 0, V = 0;
    std::vector<NlmStreamIO> table;
    std::vector<NlmCarry*> taken;   // blocks taken by this call: given back if it fails
    bool done = false;
    void read(const k2hip_model* m);
    void check(const NlmCarry* c, long long frames, const char* who, int i) const {
        const bool was = c && c->active;
        K2_REQUIRE(frames == 0 || (was == active && (!active || (c->serial == serial && c->scale == scale && c->block.carries(serial)))),
                   "%s: stream %d has searched %lld frames with another neural LM fusion setting (k2hip_set_rnn_lm_stream_fusion or "
                   "k2hip_set_rnn_lm changed it) and its hypotheses carry that LM's state -- reset the stream first", who, i, frames);
    }
    // a stream's first chunk: the start state under this call's setting
    void begin(std::unique_ptr<NlmCarry>& c) const {
        if (!c) {
            if (!active) return;
            c.reset(new NlmCarry());
        }
        c->block.release();
        c->active = active;
        c->serial = active ? serial : 0;
        c->scale = active ? scale : 0.f;
    }
    // under the engine's lock, before the launch: stream i of the call's B gets its block (first fused chunk) and its table entry
    void stage(k2hip_model* m, int i, int B, int K, NlmCarry& c);
    void flip(NlmCarry& c) const { c.block.flip(); }
    ~NlmStreamCall() {
        if (!done)
            for (NlmCarry* c : taken) c->block.release();
    }
};

// OfflineStream.cs:7-99
struct k2hip_offline_stream {
    k2hip_model* model;
    std::vector<float> speech;     // OfflineInputEntity.Speech (frame-major features) -- what has been MATERIALISED of it
    // Samples whose frames are not in `speech` yet: [the streaming fbank's left-over of the frames already materialised ; everything
    // AddSamples has accepted since].  AddSamples only appends here (no fbank launch, no lock on the model): a frame depends on its own
    // samples only (no dither, no cross-frame state), so the frames of this buffer ARE what per-call fbank would have appended, and
    // SpeechLength counts them.  GetResults hands the buffer to the engine's from-samples path (one batched fbank launch for the whole
    // batch, on the device); k2hip_offline_stream_get_speech and a batch that mixes in already materialised features run the fbank here.
    PinVec wav;
    std::vector<int64_t> tokens;   // Tokens, initialised to [blank, blank] (:34)
    std::vector<int32_t> timestamps;
    // N-best of the last k2hip_offline_recognizer_get_results made with k2hip_set_nbest(n > 1); otherwise the start state: one empty
    // alternative with score 0
    std::vector<BeamAlt> alts = std::vector<BeamAlt>(1);
    int32_t frame_offset = 0;        // FrameOffset (:39), read by the CTC search (OfflineRecognizer.cs:376,402)
    int32_t num_trailing_blank = 0;  // NumTrailingBlank (:40)
    // Input at another sample rate (k2hip_offline_stream_accept_waveform): `rate` is fixed by the stream's first samples (0: none yet),
    // `rs` is its plan (null at the model's rate).  `wav` then queues INPUT samples, wav[0] being input sample rs_x0 of the stream, and
    // rs_k0 counts the samples at the model's rate that the frames materialised or searched so far have consumed.
    int rate = 0;
    const ResamplePlan* rs = nullptr;
    int64_t rs_x0 = 0, rs_k0 = 0;
};

// OnlineStream.cs:7-199
struct k2hip_online_stream {
    k2hip_model* model;
    int slot = -1;
    std::vector<float> speech;     // OnlineInputEntity.Speech (feature FIFO)
    std::vector<float> remainder;  // streaming fbank state: samples of the last, incomplete frame shift
    // Samples accepted since the features were last materialised.  AddSamples only appends here; the fbank of
    // [remainder ; pending] runs when somebody needs the frames (the next chunk step, IsFinished, a feature read) -- for all
    // streams of a step in ONE batched launch instead of one launch per 50 ms push.  Frames depend only on their own samples
    // (no dither, no cross-frame state), so Speech is what per-call fbank would have appended; SpeechLength counts the frames
    // the pending samples will give.
    std::vector<float> pending;
    long long hyp[2] = {K2HIP_BLANK_ID, K2HIP_BLANK_ID};                 // :44
    std::vector<int64_t> tokens{K2HIP_BLANK_ID, K2HIP_BLANK_ID};         // :45
    std::vector<int32_t> timestamps;
    long long processed_len = 0;   // processed_lens state (16 per chunk)
    long long chunks_done = 0;     // chunks decoded so far: position of the stream's attention rings in its device slot
    // Device mirror of `speech` (Engine::kFifoFrames ring rows in the stream's slot): while mir_ok the ring holds exactly the frames of
    // `speech`, frame 0 at ring row mir_head, so a chunk step gathers its input on the device.  It goes stale only if the FIFO would
    // outgrow the ring; the step then reads `speech` as before, and the mirror is valid again once the FIFO has drained.
    bool mir_ok = true;
    int mir_head = 0;
    // A chunk step that failed part-way (a HIP error) may already have advanced the slot's convolution / embed caches in place (the
    // attention rings are idempotent: their position comes from chunks_done); feeding the same chunk again would then silently
    // corrupt the transcript.  Such a stream refuses every further step until k2hip_online_stream_reset.
    bool poisoned = false;
    // decoding method the stream decoded its first chunk with (-1: none yet, 0: greedy_search, K: modified_beam_search with beam K);
    // it holds until k2hip_online_stream_reset
    int method = -1;
    // modified_beam_search: the hypotheses carried between chunks; Tokens / Timestamps / Hyp are its best hypothesis
    std::unique_ptr<BeamHistory> beam;
    // ... and, under the streaming neural LM fusion, their LM state (a reset returns the block)
    std::unique_ptr<NlmCarry> nlm;
    // the stream's hotword graph (k2hip_online_stream_set_hotwords) or null; kept by a reset
    std::shared_ptr<HwResident> hw;
    // a CTC model's stream under the carried prefix search (k2hip_online_stream_set_ctc_prefix_beam; 0 = off: the per-chunk collapse);
    // the setting is kept by a reset, the prefixes are not.  Tokens / Timestamps are [blank, blank] + the best prefix
    int cp_beam = 0, cp_nbest = 1;
    std::unique_ptr<CtcPrefixHistory> cprefix;
    // k2hip_online_stream_set_ctc_prefix_biasing: the carried prefix search of this stream reads its own graph (`hw`) and the model's
    // n-gram LM.  Off by default; kept by a reset
    bool cp_biasing = false;
    // Input at another sample rate (k2hip_online_stream_accept_waveform): `rate` is fixed by the stream's first samples until a reset
    // (0: none yet), `rs` is its plan (null at the model's rate).  rs_in queues the input samples accepted since the last
    // materialisation; rs_tail is the resampler's carried input [rs_n_in - size, rs_n_in) and rs_n_in / rs_n_out its running counts
    // (resample_ref.h's state).  `pending` holds samples at the model's rate as ever: the resampler's output on its way to the fbank.
    int rate = 0;
    const ResamplePlan* rs = nullptr;
    std::vector<float> rs_in, rs_tail;
    int64_t rs_n_in = 0, rs_n_out = 0;
};

// operator level of the streaming beam search: one stream's hypotheses, fed encoder frames by the caller (k2hip_beam_search_chunk)
struct k2hip_beam_stream {
    k2hip_model* model;
    BeamHistory hist;
    std::shared_ptr<HwResident> hw;   // the stream's hotword graph (k2hip_beam_stream_set_hotwords) or null
    std::unique_ptr<NlmCarry> nlm;    // streaming neural LM fusion: the noted setting and the state block, or null
};

void NlmStreamCall::read(const k2hip_model* m) {
    active = m->engine.rnn_lm_stream_fusion_active();
    serial = m->rnn_serial;
    scale = m->rnn_scale;
    if (active) {
        L = m->rnn_lm->L; H = m->rnn_lm->H; V = m->rnn_lm->V;
    }
}
void NlmStreamCall::stage(k2hip_model* m, int i, int B, int K, NlmCarry& c) {
    if (table.empty()) table.resize((size_t)B);
    if (!c.block.held()) {
        if (!m->nlm_pool) {
            Engine* e = &m->engine;
            m->nlm_pool = std::make_shared<NlmStreamPool>([e](size_t n) { return e->dev_alloc((int64_t)n); }, [e](void* p) { e->dev_free(p); });
        }
        NlmStreamPool::take(m->nlm_pool, c.block, NlmStreamLayout{K, L, H, V}, serial);
        taken.push_back(&c);
    }
    table[(size_t)i].rd = c.block.read_half();
    table[(size_t)i].wr = c.block.write_half();
}

// operator level of the streaming CTC prefix beam search: one stream's live prefixes (k2hip_ctc_prefix_beam_search_chunk)
struct k2hip_ctc_prefix_stream {
    k2hip_model* model;
    CtcPrefixHistory hist;
    std::shared_ptr<HwResident> hw;   // the stream's hotword graph (k2hip_ctc_prefix_stream_set_hotwords) or null; read only with the switch on
    bool biasing = false;             // k2hip_ctc_prefix_stream_set_biasing; both are kept by a reset
};

// What the biased carried prefix search of one call needs beside the in / out blocks (k2hip_ctc_prefix_beam_search_chunk and the cp_beam
// branch of k2hip_online_step share it): the LM setting the call runs with, the streams' graphs and side blocks.  Unbiased streams of a
// biased call get null tables and a clear LM flag: bit for bit the plain search.
struct CtcPrefixBiasCall {
    uint64_t lm_serial = 0;
    int lm_start = 0, lm_states = 0;
    std::vector<BeamHwStream> graphs;
    std::vector<int> side_in, side_out;
    bool with_lm() const { return lm_serial != 0; }
    // before anything of any stream moves: a biased stream keeps the LM setting it searched its first chunk with
    static void check_lm(const CtcPrefixHistory& h, uint64_t lm_serial, const char* who, int i) {
        K2_REQUIRE(h.frames() == 0 || h.lm_serial() == lm_serial,
                   "%s: stream %d has searched %lld frames with another n-gram LM setting (k2hip_set_ngram_lm changed or cleared it) and its "
                   "prefixes carry that LM's states -- reset the stream first", who, i, h.frames());
    }
    void stage(int B, int K) {
        const CtcPrefixResumeBiasLayout SL{K};
        graphs.assign((size_t)B, BeamHwStream{});
        side_in.assign((size_t)B * SL.in_ints(), 0);
        side_out.assign((size_t)B * SL.out_ints(), 0);
    }
    static int graph_states(const HwResident* hw, bool biased) { return biased && hw && hw->pending ? (int)hw->pending->size() : 0; }
    void fill(int b, int K, CtcPrefixHistory& h, const HwResident* hw, bool biased) {
        const CtcPrefixResumeBiasLayout SL{K};
        if (biased && h.frames() == 0) h.begin_lm(lm_serial, with_lm(), lm_start);
        if (biased && hw) graphs[(size_t)b] = hw->tables;
        h.fill_side_in(side_in.data() + (size_t)b * SL.in_ints(), graph_states(hw, biased), biased && with_lm() ? lm_states : 0);
    }
};

// one stream's encoder caches as the operator-level API sees them (IOnlineProj's List<List<float[]>>): a slot of the device pool
// plus the two scalars of the state that live on the host (processed_lens, ring position)
struct k2hip_online_state {
    k2hip_model* model;
    int slot = -1;
    long long processed_len = 0;
    long long chunks_done = 0;
    bool poisoned = false;  // as k2hip_online_stream::poisoned: a failed EncoderProj leaves the caches undefined; destroy and re-create
};

namespace {

thread_local std::string g_last_error;

template <typename F>
int32_t guard(F&& f) {
    try {
        f();
        return K2HIP_OK;
    } catch (const Error& e) {
        g_last_error = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        g_last_error = "out of host memory";
        return K2HIP_ERR_INVALID;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return K2HIP_ERR_INVALID;
    } catch (...) {
        g_last_error = "unknown error";
        return K2HIP_ERR_INVALID;
    }
}

#define NEED(p)                                                        \
    do {                                                               \
        if (!(p)) failf(K2HIP_ERR_INVALID, "%s: null argument '%s'", __func__, #p); \
    } while (0)

}  // namespace

extern "C" {

const char* k2hip_version(void) { return "k2hip 0.1.0 (gfx950)"; }
const char* k2hip_last_error(void) { return g_last_error.c_str(); }

int32_t k2hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// "path.k2w" | "path.k2w@N" (include/k2hip.h)
static void parse_model_spec(const char* spec, std::string* path, int* device) {
    const std::string s(spec);
    *path = s;
    *device = 0;
    const size_t at = s.rfind('@');
    if (at == std::string::npos || at == 0 || at + 1 >= s.size() || s.size() - at - 1 > 4) return;   // (at most four digits)
    int d = 0;
    for (size_t i = at + 1; i < s.size(); i++) {
        if (s[i] < '0' || s[i] > '9') return;
        d = d * 10 + (s[i] - '0');
    }
    *path = s.substr(0, at);
    *device = d;
}
int32_t k2hip_parse_model_spec(const char* spec, char* path, int32_t cap, int32_t* device) {
    return guard([&] {
        NEED(spec); NEED(path); NEED(device);
        std::string p;
        int d = 0;
        parse_model_spec(spec, &p, &d);
        if ((int64_t)p.size() + 1 > (int64_t)cap) failf(K2HIP_ERR_CAPACITY, "model spec: the path needs %zu bytes", p.size() + 1);
        memcpy(path, p.c_str(), p.size() + 1);
        *device = d;
    });
}
int32_t k2hip_model_create_spec(const char* spec, const char* overrides, k2hip_model_t** out) {
    if (!spec) return k2hip_model_create(nullptr, overrides, 0, out);
    std::string p;
    int d = 0;
    parse_model_spec(spec, &p, &d);
    return k2hip_model_create(p.c_str(), overrides, d, out);
}
int32_t k2hip_model_create(const char* weights_path, const char* overrides, int32_t device, k2hip_model_t** out) {
    return guard([&] {
        NEED(weights_path);
        NEED(out);
        *out = nullptr;
        *out = new k2hip_model(weights_path, overrides, device);
    });
}
int32_t k2hip_model_destroy(k2hip_model_t* model) {
    return guard([&] { delete model; });
}
int32_t k2hip_model_get_info(const k2hip_model_t* model, k2hip_model_info* info) {
    return guard([&] {
        NEED(model);
        NEED(info);
        const Config& c = model->engine.model().cfg();
        info->vocab_size = c.V;
        info->context_size = c.ctx;
        info->joiner_dim = c.J;
        info->reserved = c.enc_dim();  // width of the encoder entry points' output (vocab_size for zipformer2ctc)
        info->feature_dim = c.feat;
        info->sample_rate = c.fbank.sample_rate;
        info->num_stacks = c.ns;
        info->device = model->engine.model().device();
    });
}
int32_t k2hip_model_meta(const k2hip_model_t* model, const char* key, char* buf, int32_t cap) {
    return guard([&] {
        NEED(model);
        NEED(key);
        NEED(buf);
        auto& mm = model->engine.model().meta();
        auto it = mm.find(key);
        if (it == mm.end()) failf(K2HIP_ERR_INVALID, "metadata key '%s' not present", key);
        if ((int)it->second.size() + 1 > cap) failf(K2HIP_ERR_CAPACITY, "metadata value needs %zu bytes", it->second.size() + 1);
        memcpy(buf, it->second.c_str(), it->second.size() + 1);
    });
}
int32_t k2hip_get_gemm_profile(k2hip_model_t* model, float* rows, int32_t cap_rows, int32_t* n_rows) {
    return guard([&] {
        NEED(model); NEED(n_rows);
        EngineLock lk(model->engine);
        const auto& lg = model->engine.gemm_log();
        *n_rows = (int32_t)lg.size();
        if (!rows) return;
        for (int i = 0; i < std::min<int>(cap_rows, (int)lg.size()); i++) {
            const GemmLaunchRec& r = lg[i];
            float* o = rows + (size_t)i * 8;
            o[0] = (float)r.M; o[1] = (float)r.N; o[2] = (float)r.K; o[3] = (float)r.batch;
            o[4] = (float)r.act; o[5] = (float)r.res; o[6] = (float)r.kind; o[7] = r.us;
        }
    });
}
int32_t k2hip_set_instrument(k2hip_model_t* model, int32_t on) {
    return guard([&] {
        NEED(model);
        EngineLock lk(model->engine);
        model->engine.set_instrument(on != 0);
    });
}
int32_t k2hip_get_timing(const k2hip_model_t* model, k2hip_timing* timing) {
    return guard([&] {
        NEED(model);
        NEED(timing);
        *timing = model->engine.timing();
    });
}

int64_t k2hip_fbank_num_frames(const k2hip_model_t* model, int64_t n_samples) {
    if (!model) return -1;
    return model->engine.fbank_num_frames(n_samples);
}
int32_t k2hip_fbank(k2hip_model_t* model, const float* samples, int64_t n_samples, float* feats, int64_t cap_frames,
                    int64_t* n_frames) {
    return guard([&] {
        NEED(model);
        NEED(n_frames);
        if (n_samples > 0) NEED(samples);
        if (cap_frames > 0) NEED(feats);
        EngineLock lk(model->engine);
        model->engine.fbank_host(samples, n_samples, feats, cap_frames, n_frames);
    });
}
int32_t k2hip_pad_sequence(k2hip_model_t* model, const float* const* speech, const int64_t* n_floats, int32_t B,
                           int32_t tail_frames, float* out, int64_t cap_floats, int64_t* padded_len) {
    return guard([&] {
        NEED(model);
        NEED(speech);
        NEED(n_floats);
        NEED(out);
        NEED(padded_len);
        EngineLock lk(model->engine);
        model->engine.pad_host(speech, n_floats, B, tail_frames, out, cap_floats, padded_len);
    });
}
int32_t k2hip_encoder_out_frames(const k2hip_model_t* model, int32_t T) {
    if (!model) return -1;
    return model->engine.encoder_out_frames(T);
}
int32_t k2hip_offline_encoder(k2hip_model_t* model, const float* x, const int64_t* x_lens, int32_t B, int32_t T,
                              float* enc_out, int64_t cap_floats, int64_t* enc_out_lens, int32_t* Tprime) {
    return guard([&] {
        NEED(model);
        NEED(x);
        NEED(enc_out);
        NEED(Tprime);
        (void)x_lens;  // always T in the reference (OfflineProjOfTransducer.cs:66-70); no masking on this path
        EngineLock lk(model->engine);
        int tp = 0;
        model->engine.encoder_host(x, B, T, enc_out, cap_floats, &tp);
        *Tprime = tp;
        if (enc_out_lens)
            for (int b = 0; b < B; b++) enc_out_lens[b] = tp;
    });
}
int32_t k2hip_offline_encoder_tap(k2hip_model_t* model, const float* x, int32_t B, int32_t T, int32_t tap, float* out,
                                  int64_t cap_floats, int64_t* n_floats) {
    return guard([&] {
        NEED(model);
        NEED(x);
        NEED(out);
        NEED(n_floats);
        EngineLock lk(model->engine);
        model->engine.encoder_tap_host(x, B, T, tap, out, cap_floats, n_floats);
    });
}
int32_t k2hip_decoder(k2hip_model_t* model, const int64_t* y, int32_t N, float* dec_out) {
    return guard([&] {
        NEED(model);
        NEED(dec_out);
        EngineLock lk(model->engine);
        model->engine.decoder_host(y, N, dec_out);
    });
}
int32_t k2hip_joiner(k2hip_model_t* model, const float* enc, const float* dec, int32_t N, float* logits) {
    return guard([&] {
        NEED(model);
        NEED(enc);
        NEED(dec);
        NEED(logits);
        EngineLock lk(model->engine);
        model->engine.joiner_host(enc, dec, N, logits);
    });
}
int32_t k2hip_greedy_batch(k2hip_model_t* model, const float* enc_out, int32_t B, int32_t Tprime, int64_t* tokens,
                           int32_t* timestamps, int32_t* n_tokens, int32_t max_tokens) {
    return guard([&] {
        NEED(model); NEED(enc_out); NEED(tokens); NEED(timestamps); NEED(n_tokens);
        EngineLock lk(model->engine);
        model->engine.greedy_host(enc_out, B, Tprime, false, tokens, timestamps, n_tokens, max_tokens);
    });
}
int32_t k2hip_greedy_single(k2hip_model_t* model, const float* enc_out, int32_t Tprime, int64_t* tokens,
                            int32_t* timestamps, int32_t* n_tokens, int32_t max_tokens) {
    return guard([&] {
        NEED(model); NEED(enc_out); NEED(tokens); NEED(timestamps); NEED(n_tokens);
        EngineLock lk(model->engine);
        model->engine.greedy_host(enc_out, 1, Tprime, true, tokens, timestamps, n_tokens, max_tokens);
    });
}
// ---- token ids -> text (text.cpp) ----------------------------------------------------------------
struct k2hip_tokens {
    k2hip::TokenTable* tab;
};
int32_t k2hip_tokens_load(const char* tokens_path, k2hip_tokens_t** out) {
    return guard([&] {
        NEED(tokens_path); NEED(out);
        auto* t = new k2hip_tokens{token_table_load(tokens_path)};
        *out = t;
    });
}
int32_t k2hip_tokens_destroy(k2hip_tokens_t* t) {
    return guard([&] {
        if (t) {
            token_table_free(t->tab);
            delete t;
        }
    });
}
int32_t k2hip_tokens_size(const k2hip_tokens_t* t) { return t ? token_table_size(t->tab) : -1; }
int32_t k2hip_bbpe_char(int32_t byte) { return bbpe_char_of_byte(byte); }
int32_t k2hip_bbpe_byte(int32_t code_point) { return code_point < 0 ? -1 : bbpe_byte_of_char((uint32_t)code_point); }
int32_t k2hip_decode_text(const k2hip_tokens_t* t, const int64_t* ids, int32_t n, int32_t online, char* out, int32_t cap,
                          int32_t* len) {
    return guard([&] {
        NEED(t); NEED(len);
        K2_REQUIRE(n == 0 || ids != nullptr, "decode_text: ids is NULL");
        std::string s = decode_tokens(*t->tab, ids, n, online != 0);
        *len = (int32_t)s.size();
        if (!out) return;
        if ((int32_t)s.size() + 1 > cap) failf(K2HIP_ERR_CAPACITY, "decode_text: text needs %zu bytes", s.size() + 1);
        memcpy(out, s.c_str(), s.size() + 1);
    });
}
// ---- hotword biasing (hotwords.cpp) ----------------------------------------------------------------
struct k2hip_hotwords {
    k2hip::HotwordGraph graph;
    uint64_t serial = ++g_hw_serial;   // the graph's identity for the models' caches (a handle's address can be reused)
};
// last reference gone (a stream detached, was reset to none or destroyed): free the tables unless the model already did
static void hw_resident_release(HwResident* r) {
    {
        std::lock_guard<std::mutex> g(g_hw_mu);
        if (r->owner) {
            auto it = r->owner->hw_cache.find(r->serial);
            if (it != r->owner->hw_cache.end() && it->second.expired()) r->owner->hw_cache.erase(it);
            try {
                Engine& e = r->owner->engine;
                EngineLock lk(e);
                e.synchronize();
                e.dev_free(r->dev);
            } catch (...) {
            }
        }
    }
    delete r;
}
// the model's resident copy of `hw`: the cached one, or a fresh upload
static std::shared_ptr<HwResident> hw_resident_get(k2hip_model* model, const k2hip_hotwords* hw, const char* who) {
    Engine& e = model->engine;
    const int V = e.model().cfg().V;
    K2_REQUIRE(hw->graph.vocab_size() == V, "%s: the graph was built for vocab_size %d, the model has %d", who, hw->graph.vocab_size(), V);
    std::lock_guard<std::mutex> g(g_hw_mu);
    auto it = model->hw_cache.find(hw->serial);
    if (it != model->hw_cache.end())
        if (auto r = it->second.lock()) return r;
    std::vector<int32_t> next;
    std::vector<float> bonus;
    auto pending = std::make_shared<std::vector<float>>();
    hw->graph.dense(&next, &bonus, pending.get());
    const int64_t nb_t = (int64_t)sizeof(int32_t) * (int64_t)next.size(), nb_p = (int64_t)sizeof(float) * (int64_t)pending->size();
    std::unique_ptr<HwResident> fresh(new HwResident());
    fresh->serial = hw->serial;
    fresh->pending = pending;
    {
        EngineLock lk(e);
        void* d = e.dev_alloc(2 * nb_t + nb_p);
        try {
            char* c = static_cast<char*>(d);
            e.dev_upload(c, next.data(), nb_t);
            e.dev_upload(c + nb_t, bonus.data(), nb_t);
            e.dev_upload(c + 2 * nb_t, pending->data(), nb_p);
            fresh->tables = BeamHwStream{reinterpret_cast<const int*>(c), reinterpret_cast<const float*>(c + nb_t),
                                         reinterpret_cast<const float*>(c + 2 * nb_t)};
        } catch (...) {
            try { e.dev_free(d); } catch (...) {}
            throw;
        }
        fresh->dev = d;
    }
    fresh->owner = model;
    std::shared_ptr<HwResident> r(fresh.release(), hw_resident_release);
    model->hw_cache[hw->serial] = r;
    model->hw_uploads++;
    return r;
}
int32_t k2hip_hotwords_create(const int64_t* ids, const int32_t* lens, int32_t n_phrases, float score_per_token, int32_t vocab_size,
                              k2hip_hotwords_t** out) {
    return guard([&] {
        NEED(out);
        *out = nullptr;
        *out = new k2hip_hotwords{HotwordGraph(ids, lens, n_phrases, score_per_token, vocab_size)};
    });
}
int32_t k2hip_hotwords_load(const k2hip_tokens_t* tokens, const char* path, float score_per_token, k2hip_hotwords_t** out) {
    return guard([&] {
        NEED(tokens); NEED(path); NEED(out);
        *out = nullptr;
        const int V = token_table_size(tokens->tab);
        std::map<std::string, int> id_of;
        for (int i = V - 1; i >= 0; i--) id_of[token_table_symbol(*tokens->tab, i)] = i;   // (a repeated symbol: its first line)
        std::ifstream f(path, std::ios::binary);
        if (!f) failf(K2HIP_ERR_IO, "cannot open hotwords file %s", path);
        std::vector<int64_t> ids;
        std::vector<int32_t> lens;
        std::vector<int> line_of;
        std::string line;
        for (int ln = 1; std::getline(f, line); ln++) {
            int n = 0;
            size_t i = 0;
            while (i < line.size()) {
                while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) i++;
                size_t j = i;
                while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') j++;
                if (j == i) break;
                const std::string sym = line.substr(i, j - i);
                auto it = id_of.find(sym);
                if (it == id_of.end()) failf(K2HIP_ERR_INVALID, "hotwords file %s line %d: token '%s' is not in the token table", path, ln, sym.c_str());
                ids.push_back(it->second);
                n++;
                i = j;
            }
            if (n == 0) continue;
            lens.push_back(n);
            line_of.push_back(ln);
        }
        *out = new k2hip_hotwords{HotwordGraph(ids.data(), lens.data(), (int)lens.size(), score_per_token, V, "line", line_of.data())};
    });
}
int32_t k2hip_hotwords_destroy(k2hip_hotwords_t* hw) {
    return guard([&] { delete hw; });
}
int32_t k2hip_hotwords_num_states(const k2hip_hotwords_t* hw) { return hw ? hw->graph.num_states() : -1; }
int32_t k2hip_hotwords_step(const k2hip_hotwords_t* hw, int32_t state, int64_t token, int32_t* next_state, float* bonus) {
    return guard([&] {
        NEED(hw); NEED(next_state); NEED(bonus);
        int n = 0;
        hw->graph.step(state, token, &n, bonus);
        *next_state = n;
    });
}
int32_t k2hip_hotwords_pending(const k2hip_hotwords_t* hw, int32_t state, float* pending) {
    return guard([&] {
        NEED(hw); NEED(pending);
        K2_REQUIRE(state >= 0 && state < hw->graph.num_states(), "hotwords: state %d outside [0, %d)", state, hw->graph.num_states());
        *pending = hw->graph.pending(state);
    });
}
int32_t k2hip_set_hotwords(k2hip_model_t* model, const k2hip_hotwords_t* hw) {
    return guard([&] {
        NEED(model);
        Engine& e = model->engine;
        const int V = e.model().cfg().V;
        if (hw) K2_REQUIRE(hw->graph.vocab_size() == V, "set_hotwords: the graph was built for vocab_size %d, the model has %d", hw->graph.vocab_size(), V);
        EngineLock lk(e);
        K2_REQUIRE(e.batches_in_flight() == 0, "set_hotwords: %d submitted batches are in flight; wait for them first", e.batches_in_flight());
        void* fresh = nullptr;
        const int32_t* d_next = nullptr;
        const float *d_bonus = nullptr, *d_pending = nullptr;
        if (hw) {
            std::vector<int32_t> next;
            std::vector<float> bonus, pending;
            hw->graph.dense(&next, &bonus, &pending);
            const int64_t nb_t = (int64_t)sizeof(int32_t) * (int64_t)next.size(), nb_p = (int64_t)sizeof(float) * (int64_t)pending.size();
            fresh = e.dev_alloc(2 * nb_t + nb_p);
            try {
                char* d = static_cast<char*>(fresh);
                e.dev_upload(d, next.data(), nb_t);
                e.dev_upload(d + nb_t, bonus.data(), nb_t);
                e.dev_upload(d + 2 * nb_t, pending.data(), nb_p);
                d_next = reinterpret_cast<const int32_t*>(d);
                d_bonus = reinterpret_cast<const float*>(d + nb_t);
                d_pending = reinterpret_cast<const float*>(d + 2 * nb_t);
            } catch (...) {
                try { e.dev_free(fresh); } catch (...) {}
                throw;
            }
        }
        // searches already enqueued read the old tables: let them finish before the memory goes
        if (model->hw_dev) {
            try {
                e.synchronize();
            } catch (...) {
                if (fresh) {
                    try { e.dev_free(fresh); } catch (...) {}
                }
                throw;
            }
        }
        e.set_hotword_tables(d_next, d_bonus, d_pending);
        void* old = model->hw_dev;
        model->hw_dev = fresh;
        if (old) e.dev_free(old);
    });
}
// ---- keyword spotting (keywords.cpp, kws.hip) -----------------------------------------------------------
// What the CTC spotter reads of a graph: the graph itself, rc(s) = the root's child whose token is tok(s) (or -1) and the table block
// the engine uploads.  Built with the handle and shared by its CTC streams, which keep it alive after the handle is gone; streams of
// one call that share it share one upload.
struct CtcKwShared {
    std::shared_ptr<const KeywordGraph> graph;
    std::vector<int32_t> rc;
    Engine::CtcKwsGraph tables;
    explicit CtcKwShared(std::shared_ptr<const KeywordGraph> g) : graph(std::move(g)), rc((size_t)graph->num_states()) {
        const KeywordGraph& k = *graph;
        ctc_kws_root_children(k.parent().data(), k.tok().data(), k.num_states(), rc.data());
        tables = Engine::CtcKwsGraph{k.parent().data(), k.tok().data(), k.depth().data(), k.kw().data(), k.bar().data(), rc.data(), k.num_states()};
    }
};
struct k2hip_keywords {
    std::shared_ptr<const KeywordGraph> graph;
    uint64_t serial = ++g_hw_serial;   // the graph's identity for the models' caches (a handle's address can be reused)
    std::shared_ptr<const CtcKwShared> ctc = std::make_shared<const CtcKwShared>(graph);
};
// last reference gone: free the resident block unless the model already did
static void kw_resident_release(KwResident* r) {
    {
        std::lock_guard<std::mutex> g(g_hw_mu);
        if (r->owner) {
            auto it = r->owner->kw_cache.find(r->serial);
            if (it != r->owner->kw_cache.end() && it->second.expired()) r->owner->kw_cache.erase(it);
            try {
                Engine& e = r->owner->engine;
                EngineLock lk(e);
                e.synchronize();
                e.dev_free(r->dev);
            } catch (...) {
            }
        }
    }
    delete r;
}
// the model's resident copy of `kw`: the cached one, or a fresh upload (its decoder rows are computed here, once)
static std::shared_ptr<KwResident> kw_resident_get(k2hip_model* model, const k2hip_keywords* kw, const char* who) {
    Engine& e = model->engine;
    const Config& cf = e.model().cfg();
    if (cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "%s: a CTC model has no transducer lattice", who);
    K2_REQUIRE(kw->graph->vocab_size() == cf.V, "%s: the graph was built for vocab_size %d, the model has %d", who, kw->graph->vocab_size(), cf.V);
    std::lock_guard<std::mutex> g(g_hw_mu);
    auto it = model->kw_cache.find(kw->serial);
    if (it != model->kw_cache.end())
        if (auto r = it->second.lock()) return r;
    std::unique_ptr<KwResident> fresh(new KwResident());
    fresh->serial = kw->serial;
    fresh->graph = kw->graph;
    {
        EngineLock lk(e);
        fresh->dev = e.kws_graph_upload(*kw->graph, &fresh->tables);
    }
    fresh->owner = model;
    std::shared_ptr<KwResident> r(fresh.release(), kw_resident_release);
    model->kw_cache[kw->serial] = r;
    return r;
}
int32_t k2hip_keywords_create(const int64_t* ids, const int32_t* lens, const float* thresholds, int32_t n_keywords, int32_t vocab_size,
                              k2hip_keywords_t** out) {
    return guard([&] {
        NEED(out);
        *out = nullptr;
        auto g = std::make_shared<const KeywordGraph>(ids, lens, thresholds, n_keywords, vocab_size);
        *out = new k2hip_keywords{std::move(g)};
    });
}
int32_t k2hip_keywords_load(const k2hip_tokens_t* tokens, const char* path, float default_threshold, k2hip_keywords_t** out) {
    return guard([&] {
        NEED(tokens); NEED(path); NEED(out);
        *out = nullptr;
        const int V = token_table_size(tokens->tab);
        std::map<std::string, int> id_of;
        for (int i = V - 1; i >= 0; i--) id_of[token_table_symbol(*tokens->tab, i)] = i;   // (a repeated symbol: its first line)
        std::ifstream f(path, std::ios::binary);
        if (!f) failf(K2HIP_ERR_IO, "cannot open keywords file %s", path);
        std::vector<int64_t> ids;
        std::vector<int32_t> lens;
        std::vector<float> thr;
        std::vector<int> line_of;
        std::string line;
        for (int ln = 1; std::getline(f, line); ln++) {
            std::vector<std::string> fields;
            size_t i = 0;
            while (i < line.size()) {
                while (i < line.size() && (line[i] == ' ' || line[i] == '\t' || line[i] == '\r')) i++;
                size_t j = i;
                while (j < line.size() && line[j] != ' ' && line[j] != '\t' && line[j] != '\r') j++;
                if (j == i) break;
                fields.push_back(line.substr(i, j - i));
                i = j;
            }
            if (fields.empty()) continue;
            float th = default_threshold;
            // a last field ":<number>" that is no token of the table is the line's threshold
            const std::string& last = fields.back();
            if (last.size() > 1 && last[0] == ':' && id_of.find(last) == id_of.end()) {
                char* endp = nullptr;
                th = strtof(last.c_str() + 1, &endp);
                if (endp == last.c_str() + 1 || *endp != '\0')
                    failf(K2HIP_ERR_INVALID, "keywords file %s line %d: threshold '%s' is not a number", path, ln, last.c_str());
                fields.pop_back();
            }
            for (const std::string& sym : fields) {
                auto it = id_of.find(sym);
                if (it == id_of.end()) failf(K2HIP_ERR_INVALID, "keywords file %s line %d: token '%s' is not in the token table", path, ln, sym.c_str());
                ids.push_back(it->second);
            }
            lens.push_back((int32_t)fields.size());
            thr.push_back(th);
            line_of.push_back(ln);
        }
        auto g = std::make_shared<const KeywordGraph>(ids.data(), lens.data(), thr.data(), (int)lens.size(), V, "line", line_of.data());
        *out = new k2hip_keywords{std::move(g)};
    });
}
int32_t k2hip_keywords_destroy(k2hip_keywords_t* kw) {
    return guard([&] { delete kw; });
}
int32_t k2hip_keywords_num_states(const k2hip_keywords_t* kw) { return kw ? kw->graph->num_states() : -1; }
int32_t k2hip_keywords_num_keywords(const k2hip_keywords_t* kw) { return kw ? kw->graph->num_keywords() : -1; }
int32_t k2hip_debug_keywords_get_tables(const k2hip_keywords_t* kw, int32_t* parent, int32_t* tok, int32_t* depth, int32_t* keyword, float* bar,
                                        int32_t cap) {
    return guard([&] {
        NEED(kw);
        const KeywordGraph& g = *kw->graph;
        const size_t S = (size_t)g.num_states();
        if ((int64_t)S > cap) failf(K2HIP_ERR_CAPACITY, "the graph has %zu states", S);
        if (parent) memcpy(parent, g.parent().data(), 4 * S);
        if (tok) memcpy(tok, g.tok().data(), 4 * S);
        if (depth) memcpy(depth, g.depth().data(), 4 * S);
        if (keyword) memcpy(keyword, g.kw().data(), 4 * S);
        if (bar) memcpy(bar, g.bar().data(), 4 * S);
    });
}
// the events of a k2hip_debug_*_ref_dp call into the caller's arrays
static void kws_ref_events_out(const std::vector<KwsRefEvent>& ev, const char* who, int32_t* ev_keyword, int32_t* ev_start, int32_t* ev_end, float* ev_sum,
                               int32_t cap, int32_t* n_events) {
    *n_events = (int32_t)ev.size();
    if ((int64_t)ev.size() > cap) failf(K2HIP_ERR_CAPACITY, "%s: %zu events", who, ev.size());
    for (size_t i = 0; i < ev.size(); i++) {
        if (ev_keyword) ev_keyword[i] = ev[i].keyword;
        if (ev_start) ev_start[i] = ev[i].start;
        if (ev_end) ev_end[i] = ev[i].end;
        if (ev_sum) ev_sum[i] = ev[i].sum_logp;
    }
}
int32_t k2hip_debug_kws_ref_dp(const int32_t* parent, const int32_t* depth, const int32_t* keyword, const float* bar, int32_t S, const float* stay,
                               const float* emit, int32_t T, float* a, int32_t* start, int32_t* ev_keyword, int32_t* ev_start, int32_t* ev_end,
                               float* ev_sum, int32_t cap, int32_t* n_events) {
    return guard([&] {
        NEED(parent); NEED(depth); NEED(keyword); NEED(bar); NEED(a); NEED(start); NEED(n_events);
        K2_REQUIRE(S >= 1 && T >= 0 && cap >= 0, "kws_ref_dp: bad shape S=%d T=%d", S, T);
        K2_REQUIRE(T == 0 || S == 1 || (stay && emit), "kws_ref_dp: null planes");
        for (int s = 1; s < S; s++) K2_REQUIRE(parent[s] >= 0 && parent[s] < s, "kws_ref_dp: parent(%d) = %d", s, parent[s]);
        std::vector<KwsRefEvent> ev;
        kws_dp_ref(parent, depth, keyword, bar, S, stay, emit, T, a, start, &ev);
        kws_ref_events_out(ev, "kws_ref_dp", ev_keyword, ev_start, ev_end, ev_sum, cap, n_events);
    });
}
int32_t k2hip_debug_ctc_kws_ref_dp(const int32_t* parent, const int32_t* tok, const int32_t* depth, const int32_t* keyword, const float* bar,
                                   const int32_t* rc, int32_t S, const float* log_probs, int32_t V, int32_t T, float* v, int32_t* st,
                                   int32_t* ev_keyword, int32_t* ev_start, int32_t* ev_end, float* ev_sum, int32_t cap, int32_t* n_events) {
    return guard([&] {
        NEED(parent); NEED(tok); NEED(depth); NEED(keyword); NEED(bar); NEED(rc); NEED(v); NEED(st); NEED(n_events);
        K2_REQUIRE(S >= 1 && T >= 0 && V >= 2 && cap >= 0, "ctc_kws_ref_dp: bad shape S=%d T=%d V=%d", S, T, V);
        K2_REQUIRE(T == 0 || log_probs, "ctc_kws_ref_dp: null log_probs");
        for (int s = 1; s < S; s++) {
            K2_REQUIRE(parent[s] >= 0 && parent[s] < s, "ctc_kws_ref_dp: parent(%d) = %d", s, parent[s]);
            K2_REQUIRE(tok[s] >= 1 && tok[s] < V, "ctc_kws_ref_dp: tok(%d) = %d", s, tok[s]);
            K2_REQUIRE(rc[s] == -1 || (rc[s] >= 1 && rc[s] < S && parent[rc[s]] == 0), "ctc_kws_ref_dp: rc(%d) = %d", s, rc[s]);
        }
        K2_REQUIRE(st[S] == -1 || (st[S] >= 1 && st[S] < S && parent[st[S]] == 0), "ctc_kws_ref_dp: hold = %d", st[S]);
        std::vector<KwsRefEvent> ev;
        ctc_kws_dp_ref(parent, tok, depth, keyword, bar, rc, S, log_probs, V, T, v, st, &ev);
        kws_ref_events_out(ev, "ctc_kws_ref_dp", ev_keyword, ev_start, ev_end, ev_sum, cap, n_events);
    });
}
// the refusals every CTC spotting entry shares, decided on the host
static void ctc_kws_check(k2hip_model* model, const k2hip_keywords* kw, const char* who) {
    const Config& cf = model->engine.model().cfg();
    if (!cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "%s: model_type '%s' has no CTC head", who, cf.model_type.c_str());
    if (kw) K2_REQUIRE(kw->graph->vocab_size() == cf.V, "%s: the graph was built for vocab_size %d, the model has %d", who, kw->graph->vocab_size(), cf.V);
}
}  // extern "C"

// ---- the keyword streams of both spotters (kws.hip, ctc_kws.hip): one implementation --------------------------------------------
// What differs between the two is named by a spotter: the graph holder its streams keep alive, the carried block's width per trie state
// and its fresh state, the refusals decided on the host and the engine's two calls.  The stream, its bookkeeping and the chunk and
// fused entries' checks, write-back and copy-out are written once over it; the exported entries below check their pointers and pass
// their own name `who` for the messages.
struct LatticeSpotter {   // transducer models: the carried block is a / start [S] (kws_ref.h)
    using Holder = KwResident;
    using IO = Engine::KwsIO;
    static constexpr int kWidth = 1;
    static constexpr const char* kStateFull = "the stream's graph has %zu states";
    static std::shared_ptr<Holder> holder(k2hip_model* model, const k2hip_keywords* kw, const char* who) { return kw_resident_get(model, kw, who); }
    static void check_model(k2hip_model* model, const char* who) {
        if (model->engine.model().cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "%s: a CTC model has no transducer lattice", who);
    }
    static void fresh_state(int S, float* val, int32_t* st) { kws_fresh_state(S, val, st); }
    static void chunk(Engine& e, const float* enc_out, int B, int Tc, const IO* io, Engine::KwsResult* r) { e.kws_chunk_host(enc_out, B, Tc, io, r); }
    static void samples(Engine& e, const float* const* samples, const int64_t* n_samples, int B, const IO* io, Engine::KwsResult* r, int32_t* Tp) {
        e.kws_samples(samples, n_samples, B, io, r, Tp);
    }
};
struct CtcSpotter {       // CTC models: the carried block is v / st [2][S] (ctc_kws_ref.h)
    using Holder = const CtcKwShared;
    using IO = Engine::CtcKwsIO;
    static constexpr int kWidth = 2;
    static constexpr const char* kStateFull = "the stream's block has %zu cells";
    static std::shared_ptr<Holder> holder(k2hip_model* model, const k2hip_keywords* kw, const char* who) {
        ctc_kws_check(model, kw, who);
        return kw->ctc;
    }
    static void check_model(k2hip_model* model, const char* who) { ctc_kws_check(model, nullptr, who); }
    static void fresh_state(int S, float* val, int32_t* st) { ctc_kws_fresh_state(S, val, st); }
    static void chunk(Engine& e, const float* log_probs, int B, int Tc, const IO* io, Engine::KwsResult* r) { e.ctc_kws_chunk_host(log_probs, B, Tc, io, r); }
    static void samples(Engine& e, const float* const* samples, const int64_t* n_samples, int B, const IO* io, Engine::KwsResult* r, int32_t* Tp) {
        e.ctc_kws_samples(samples, n_samples, B, io, r, Tp);
    }
};
template <class K>
struct KwStream {
    using Spotter = K;
    k2hip_model* model = nullptr;
    std::shared_ptr<typename K::Holder> hold;
    std::vector<float> val;          // the carried block: kWidth * S values and as many starts; st[0] counts the stream's frames
    std::vector<int32_t> st;
    std::vector<KwsRefEvent> events;
    void fresh() {
        const int S = hold->graph->num_states();
        val.resize((size_t)K::kWidth * S);
        st.resize((size_t)K::kWidth * S);
        K::fresh_state(S, val.data(), st.data());
        events.clear();
    }
};
struct k2hip_kws_stream : KwStream<LatticeSpotter> {};
struct k2hip_ctc_kws_stream : KwStream<CtcSpotter> {};

namespace {
template <class S>
void kw_stream_create(k2hip_model* model, const k2hip_keywords* kw, S** out, const char* who) {
    *out = nullptr;
    std::unique_ptr<S> s(new S());
    s->model = model;
    s->hold = S::Spotter::holder(model, kw, who);
    s->fresh();
    *out = s.release();
}
// the events of a list through the getters' common rules; depth_of: the keyword's number of tokens
int32_t kws_events_out(const KeywordGraph& g, const KwsRefEvent* ev, size_t n, int32_t* keyword, int32_t* start, int32_t* end, float* sum_logp, float* score,
                       size_t cap) {
    const size_t m = std::min(n, cap);
    for (size_t i = 0; i < m; i++) {
        if (keyword) keyword[i] = ev[i].keyword;
        if (start) start[i] = ev[i].start;
        if (end) end[i] = ev[i].end;
        if (sum_logp) sum_logp[i] = ev[i].sum_logp;
        if (score) score[i] = ev[i].sum_logp / (float)g.depth()[(size_t)g.terminal()[(size_t)ev[i].keyword]];
    }
    return (int32_t)n;
}
template <class S>
int32_t kw_stream_get_events(const S* s, int32_t* keyword, int32_t* start, int32_t* end, float* sum_logp, float* score, int32_t cap, const char* who) {
    K2_REQUIRE(cap >= 0, "%s: cap %d", who, cap);
    return kws_events_out(*s->hold->graph, s->events.data(), s->events.size(), keyword, start, end, sum_logp, score, (size_t)cap);
}
template <class S>
void kw_stream_get_state(const S* s, float* val, int32_t* st, int32_t cap) {
    if ((int64_t)s->val.size() > cap) failf(K2HIP_ERR_CAPACITY, S::Spotter::kStateFull, s->val.size());
    if (val) memcpy(val, s->val.data(), sizeof(float) * s->val.size());
    if (st) memcpy(st, s->st.data(), sizeof(int32_t) * s->st.size());
}
// the events of row b of a chunk result behind `into`
void kws_take_events(const Engine::KwsResult& r, int b, std::vector<KwsRefEvent>* into) {
    for (int i = 0; i < r.n[(size_t)b]; i++) {
        const size_t o = (size_t)b * r.mt + i;
        into->push_back(KwsRefEvent{(int32_t)r.keyword[o], r.start[o], r.end[o], r.sum[o]});
    }
}
// x: encoder_out (transducer) or log_probs (CTC), [B][Tc][.] on the host
template <class S>
void kw_search_chunk(k2hip_model* model, S* const* streams, int32_t B, const float* x, int32_t Tc, const int32_t* n_frames, const char* who) {
    using K = typename S::Spotter;
    K2_REQUIRE(B > 0 && Tc >= 1, "%s: bad shape B=%d Tc=%d", who, B, Tc);
    K::check_model(model, who);
    Engine& e = model->engine;
    std::vector<typename K::IO> io((size_t)B);
    for (int b = 0; b < B; b++) {
        S* s = streams[b];
        K2_REQUIRE(s != nullptr, "%s: stream %d is null", who, b);
        K2_REQUIRE(s->model == model, "%s: stream %d belongs to another model", who, b);
        for (int c = 0; c < b; c++) K2_REQUIRE(streams[c] != s, "%s: streams %d and %d are the same stream", who, c, b);
        const int T = n_frames ? n_frames[b] : Tc;
        K2_REQUIRE(T >= 0 && T <= Tc, "%s: stream %d: n_frames %d outside [0, %d]", who, b, T, Tc);
        K2_REQUIRE((int64_t)s->st[0] + T <= INT32_MAX, "%s: stream %d has run out of frame numbers; reset it", who, b);
        io[(size_t)b] = typename K::IO{&s->hold->tables, T, s->val.data(), s->st.data()};
    }
    Engine::KwsResult r;
    {
        EngineLock lk(e);
        K::chunk(e, x, B, Tc, io.data(), &r);
    }
    for (int b = 0; b < B; b++) K2_REQUIRE(r.n[(size_t)b] >= 0 && r.n[(size_t)b] <= r.mt, "internal: stream %d reports %d events", b, r.n[(size_t)b]);
    // nothing below fails: the call is applied to every stream or to none
    for (int b = 0; b < B; b++) {
        S* s = streams[b];
        if (io[(size_t)b].T == 0) continue;
        const size_t n = s->val.size(), o = (size_t)K::kWidth * (size_t)r.state_off[(size_t)b];
        memcpy(s->val.data(), r.a.data() + o, sizeof(float) * n);
        memcpy(s->st.data(), r.st.data() + o, sizeof(int32_t) * n);
        kws_take_events(r, b, &s->events);
    }
}
template <class K>
void kw_spot_from_samples(k2hip_model* model, const k2hip_keywords* kw, const float* const* samples, const int64_t* n_samples, int32_t B, int32_t* keyword,
                          int32_t* start, int32_t* end, float* sum_logp, float* score, int32_t* n_events, int32_t max_events, int32_t* Tprime_out,
                          const char* who) {
    K2_REQUIRE(B > 0 && max_events >= 0, "%s: bad shape B=%d max_events=%d", who, B, max_events);
    const std::shared_ptr<typename K::Holder> hold = K::holder(model, kw, who);
    Engine& e = model->engine;
    const int S = hold->graph->num_states();
    std::vector<float> v0((size_t)K::kWidth * S);
    std::vector<int32_t> s0((size_t)K::kWidth * S);
    K::fresh_state(S, v0.data(), s0.data());
    std::vector<typename K::IO> io((size_t)B, typename K::IO{&hold->tables, 0, v0.data(), s0.data()});
    Engine::KwsResult r;
    int32_t Tp = 0;
    {
        EngineLock lk(e);
        K::samples(e, samples, n_samples, B, io.data(), &r, &Tp);
    }
    for (int b = 0; b < B; b++) {
        K2_REQUIRE(r.n[(size_t)b] >= 0 && r.n[(size_t)b] <= r.mt, "internal: stream %d reports %d events", b, r.n[(size_t)b]);
        if (r.n[(size_t)b] > max_events) failf(K2HIP_ERR_CAPACITY, "%s: stream %d has %d events, max_events is %d", who, b, r.n[(size_t)b], max_events);
    }
    for (int b = 0; b < B; b++) {
        std::vector<KwsRefEvent> ev;
        kws_take_events(r, b, &ev);
        const size_t o = (size_t)b * (size_t)max_events;
        kws_events_out(*hold->graph, ev.data(), ev.size(), keyword ? keyword + o : nullptr, start ? start + o : nullptr, end ? end + o : nullptr,
                       sum_logp ? sum_logp + o : nullptr, score ? score + o : nullptr, ev.size());
        n_events[b] = (int32_t)ev.size();
    }
    if (Tprime_out) *Tprime_out = Tp;
}
}  // namespace

extern "C" {
// ---- keyword spotting (keywords.cpp, kws.hip) and keyword spotting for CTC models (ctc_kws.hip): the exported entries -------------
int32_t k2hip_kws_stream_create(k2hip_model_t* model, const k2hip_keywords_t* kw, k2hip_kws_stream_t** out) {
    return guard([&] { NEED(model); NEED(kw); NEED(out); kw_stream_create(model, kw, out, "kws_stream_create"); });
}
int32_t k2hip_ctc_kws_stream_create(k2hip_model_t* model, const k2hip_keywords_t* kw, k2hip_ctc_kws_stream_t** out) {
    return guard([&] { NEED(model); NEED(kw); NEED(out); kw_stream_create(model, kw, out, "ctc_kws_stream_create"); });
}
int32_t k2hip_kws_stream_destroy(k2hip_kws_stream_t* s) { return guard([&] { delete s; }); }
int32_t k2hip_ctc_kws_stream_destroy(k2hip_ctc_kws_stream_t* s) { return guard([&] { delete s; }); }
int32_t k2hip_kws_stream_reset(k2hip_kws_stream_t* s) { return guard([&] { NEED(s); s->fresh(); }); }
int32_t k2hip_ctc_kws_stream_reset(k2hip_ctc_kws_stream_t* s) { return guard([&] { NEED(s); s->fresh(); }); }
int64_t k2hip_kws_stream_num_frames(const k2hip_kws_stream_t* s) { return s ? (int64_t)s->st[0] : -1; }
int64_t k2hip_ctc_kws_stream_num_frames(const k2hip_ctc_kws_stream_t* s) { return s ? (int64_t)s->st[0] : -1; }
int32_t k2hip_kws_stream_num_events(const k2hip_kws_stream_t* s) { return s ? (int32_t)s->events.size() : -1; }
int32_t k2hip_ctc_kws_stream_num_events(const k2hip_ctc_kws_stream_t* s) { return s ? (int32_t)s->events.size() : -1; }
int32_t k2hip_kws_stream_get_events(const k2hip_kws_stream_t* s, int32_t* keyword, int32_t* start, int32_t* end, float* sum_logp, float* score,
                                    int32_t cap) {
    int32_t count = 0;
    const int32_t rc = guard([&] { NEED(s); count = kw_stream_get_events(s, keyword, start, end, sum_logp, score, cap, "kws_stream_get_events"); });
    return rc < 0 ? rc : count;
}
int32_t k2hip_ctc_kws_stream_get_events(const k2hip_ctc_kws_stream_t* s, int32_t* keyword, int32_t* start, int32_t* end, float* sum_logp, float* score,
                                        int32_t cap) {
    int32_t count = 0;
    const int32_t rc = guard([&] { NEED(s); count = kw_stream_get_events(s, keyword, start, end, sum_logp, score, cap, "ctc_kws_stream_get_events"); });
    return rc < 0 ? rc : count;
}
int32_t k2hip_kws_stream_clear_events(k2hip_kws_stream_t* s) { return guard([&] { NEED(s); s->events.clear(); }); }
int32_t k2hip_ctc_kws_stream_clear_events(k2hip_ctc_kws_stream_t* s) { return guard([&] { NEED(s); s->events.clear(); }); }
int32_t k2hip_debug_kws_stream_get_state(const k2hip_kws_stream_t* s, float* a, int32_t* start, int32_t cap) {
    return guard([&] { NEED(s); kw_stream_get_state(s, a, start, cap); });
}
int32_t k2hip_debug_ctc_kws_stream_get_state(const k2hip_ctc_kws_stream_t* s, float* v, int32_t* st, int32_t cap) {
    return guard([&] { NEED(s); kw_stream_get_state(s, v, st, cap); });
}
int32_t k2hip_kws_search_chunk(k2hip_model_t* model, k2hip_kws_stream_t* const* streams, int32_t B, const float* enc_out, int32_t Tc,
                               const int32_t* n_frames) {
    return guard([&] { NEED(model); NEED(streams); NEED(enc_out); kw_search_chunk(model, streams, B, enc_out, Tc, n_frames, "kws_search_chunk"); });
}
int32_t k2hip_ctc_kws_search_chunk(k2hip_model_t* model, k2hip_ctc_kws_stream_t* const* streams, int32_t B, const float* log_probs, int32_t Tc,
                                   const int32_t* n_frames) {
    return guard([&] { NEED(model); NEED(streams); NEED(log_probs); kw_search_chunk(model, streams, B, log_probs, Tc, n_frames, "ctc_kws_search_chunk"); });
}
int32_t k2hip_offline_spot_keywords_from_samples(k2hip_model_t* model, const k2hip_keywords_t* kw, const float* const* samples,
                                                 const int64_t* n_samples, int32_t B, int32_t* keyword, int32_t* start, int32_t* end,
                                                 float* sum_logp, float* score, int32_t* n_events, int32_t max_events, int32_t* Tprime_out) {
    return guard([&] {
        NEED(model); NEED(kw); NEED(samples); NEED(n_samples); NEED(n_events);
        kw_spot_from_samples<LatticeSpotter>(model, kw, samples, n_samples, B, keyword, start, end, sum_logp, score, n_events, max_events, Tprime_out,
                                             "spot_keywords_from_samples");
    });
}
int32_t k2hip_offline_ctc_spot_keywords_from_samples(k2hip_model_t* model, const k2hip_keywords_t* kw, const float* const* samples,
                                                     const int64_t* n_samples, int32_t B, int32_t* keyword, int32_t* start, int32_t* end,
                                                     float* sum_logp, float* score, int32_t* n_events, int32_t max_events, int32_t* Tprime_out) {
    return guard([&] {
        NEED(model); NEED(kw); NEED(samples); NEED(n_samples); NEED(n_events);
        kw_spot_from_samples<CtcSpotter>(model, kw, samples, n_samples, B, keyword, start, end, sum_logp, score, n_events, max_events, Tprime_out,
                                         "ctc_spot_keywords_from_samples");
    });
}
// ---- n-gram LM shallow fusion (ngram_lm.cpp) -----------------------------------------------------------
struct k2hip_ngram_lm {
    std::unique_ptr<k2hip::NgramLm> lm;
};
int32_t k2hip_ngram_lm_create(const int64_t* ids, const int32_t* orders, const float* log_probs, const float* backoffs, int64_t n_entries,
                              int32_t vocab_size, k2hip_ngram_lm_t** out) {
    return guard([&] {
        NEED(out);
        *out = nullptr;
        std::unique_ptr<NgramLm> lm(new NgramLm(ids, orders, log_probs, backoffs, n_entries, vocab_size));
        *out = new k2hip_ngram_lm{std::move(lm)};
    });
}
int32_t k2hip_ngram_lm_load(const k2hip_tokens_t* tokens, const char* path, k2hip_ngram_lm_t** out) {
    return guard([&] {
        NEED(tokens); NEED(path); NEED(out);
        *out = nullptr;
        const int V = token_table_size(tokens->tab);
        std::map<std::string, int> id_of;
        for (int i = V - 1; i >= 0; i--) id_of[token_table_symbol(*tokens->tab, i)] = i;   // (a repeated symbol: its first line)
        std::ifstream f(path, std::ios::binary);
        if (!f) failf(K2HIP_ERR_IO, "cannot open ngram lm file %s", path);
        std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        std::unique_ptr<NgramLm> lm(ngram_parse_arpa(text.data(), text.size(), id_of, V, path));
        *out = new k2hip_ngram_lm{std::move(lm)};
    });
}
int32_t k2hip_ngram_lm_destroy(k2hip_ngram_lm_t* lm) {
    return guard([&] { delete lm; });
}
int32_t k2hip_ngram_lm_order(const k2hip_ngram_lm_t* lm) { return lm ? lm->lm->order() : -1; }
int32_t k2hip_ngram_lm_num_states(const k2hip_ngram_lm_t* lm) { return lm ? lm->lm->num_states() : -1; }
int64_t k2hip_ngram_lm_num_arcs(const k2hip_ngram_lm_t* lm) { return lm ? lm->lm->num_arcs() : -1; }
int32_t k2hip_ngram_lm_start_state(const k2hip_ngram_lm_t* lm) { return lm ? lm->lm->start_state() : -1; }
int32_t k2hip_ngram_lm_step(const k2hip_ngram_lm_t* lm, int32_t state, int64_t token, int32_t* next_state, float* log_prob) {
    return guard([&] {
        NEED(lm); NEED(next_state); NEED(log_prob);
        int n = 0;
        lm->lm->step(state, token, &n, log_prob);
        *next_state = n;
    });
}
// the scaled sparse form of an n-gram LM into ONE device allocation (returned; the caller owns it) and the kernels' view of it
static void* ngram_tables_upload(Engine& e, const NgramDeviceForm& d, int V, int start, BeamLm* out) {
    const int64_t nb_s = align_up((int64_t)sizeof(int32_t) * (int64_t)d.states.size(), 16);
    const int64_t nb_a = align_up((int64_t)sizeof(int32_t) * std::max<int64_t>((int64_t)d.arc_tok.size(), 1), 16);
    const int64_t nb_v = align_up((int64_t)sizeof(int32_t) * V, 16);
    void* fresh = e.dev_alloc(nb_s + 3 * nb_a + 2 * nb_v);
    try {
        char* c = static_cast<char*>(fresh);
        e.dev_upload(c, d.states.data(), (int64_t)sizeof(int32_t) * (int64_t)d.states.size());
        if (!d.arc_tok.empty()) {
            e.dev_upload(c + nb_s, d.arc_tok.data(), (int64_t)sizeof(int32_t) * (int64_t)d.arc_tok.size());
            e.dev_upload(c + nb_s + nb_a, d.arc_lp.data(), (int64_t)sizeof(float) * (int64_t)d.arc_lp.size());
            e.dev_upload(c + nb_s + 2 * nb_a, d.arc_next.data(), (int64_t)sizeof(int32_t) * (int64_t)d.arc_next.size());
        }
        e.dev_upload(c + nb_s + 3 * nb_a, d.uni_lp.data(), (int64_t)sizeof(float) * V);
        e.dev_upload(c + nb_s + 3 * nb_a + nb_v, d.uni_next.data(), (int64_t)sizeof(int32_t) * V);
        out->states = reinterpret_cast<const int4*>(c);
        out->arc_tok = reinterpret_cast<const int*>(c + nb_s);
        out->arc_lp = reinterpret_cast<const float*>(c + nb_s + nb_a);
        out->arc_next = reinterpret_cast<const int*>(c + nb_s + 2 * nb_a);
        out->uni_lp = reinterpret_cast<const float*>(c + nb_s + 3 * nb_a);
        out->uni_next = reinterpret_cast<const int*>(c + nb_s + 3 * nb_a + nb_v);
        out->start = start;
    } catch (...) {
        try { e.dev_free(fresh); } catch (...) {}
        throw;
    }
    return fresh;
}
int32_t k2hip_set_ngram_lm(k2hip_model_t* model, const k2hip_ngram_lm_t* lm, float scale) {
    return guard([&] {
        NEED(model);
        Engine& e = model->engine;
        const int V = e.model().cfg().V;
        if (lm) {
            K2_REQUIRE(std::isfinite(scale) && scale >= 0.f, "set_ngram_lm: scale %g must be finite and >= 0", (double)scale);
            K2_REQUIRE(lm->lm->vocab_size() == V, "set_ngram_lm: the LM was built for vocab_size %d, the model has %d", lm->lm->vocab_size(), V);
        }
        EngineLock lk(e);
        K2_REQUIRE(e.batches_in_flight() == 0, "set_ngram_lm: %d submitted batches are in flight; wait for them first", e.batches_in_flight());
        void* fresh = nullptr;
        BeamLm tables;
        int n_states = 0;
        if (lm && scale > 0.f) {   // (scale = 0 adds nothing anywhere: the plain search, as with no LM)
            NgramDeviceForm d;
            lm->lm->device_form(scale, &d);
            n_states = (int)(d.states.size() / 4);
            fresh = ngram_tables_upload(e, d, V, lm->lm->start_state(), &tables);
        }
        // searches already enqueued read the old tables: let them finish before the memory goes
        if (model->lm_dev) {
            try {
                e.synchronize();
            } catch (...) {
                if (fresh) {
                    try { e.dev_free(fresh); } catch (...) {}
                }
                throw;
            }
        }
        e.set_ngram_tables(tables);
        model->lm_serial = fresh ? ++g_hw_serial : 0;
        model->lm_start = tables.start;
        model->lm_states = fresh ? n_states : 0;
        void* old = model->lm_dev;
        model->lm_dev = fresh;
        if (old) e.dev_free(old);
    });
}
// LODR: a second automaton slot beside k2hip_set_ngram_lm's, subtracted (scale <= 0) where the neural LM is added
int32_t k2hip_set_lodr_lm(k2hip_model_t* model, const k2hip_ngram_lm_t* lm, float scale) {
    return guard([&] {
        NEED(model);
        Engine& e = model->engine;
        const int V = e.model().cfg().V;
        if (lm) {
            K2_REQUIRE(std::isfinite(scale), "set_lodr_lm: scale %g must be finite", (double)scale);
            K2_REQUIRE(scale <= 0.f, "set_lodr_lm: scale %g must be <= 0 -- the LODR weight is given as a negative number; an added n-gram "
                       "weight is k2hip_set_ngram_lm's job", (double)scale);
            K2_REQUIRE(lm->lm->vocab_size() == V, "set_lodr_lm: the LM was built for vocab_size %d, the model has %d", lm->lm->vocab_size(), V);
        }
        EngineLock lk(e);
        K2_REQUIRE(e.batches_in_flight() == 0, "set_lodr_lm: %d submitted batches are in flight; wait for them first", e.batches_in_flight());
        void* fresh = nullptr;
        BeamLm tables;
        std::unique_ptr<NgramLm> copy;
        std::shared_ptr<LodrHost> host;
        if (lm && scale < 0.f) {   // (scale = 0 subtracts nothing anywhere: as with no LODR LM)
            copy.reset(new NgramLm(*lm->lm));   // (the handle may be destroyed after this call)
            host = std::make_shared<LodrHost>();
            copy->device_form(scale, &host->d);
            host->start = copy->start_state();
            host->V = V;
            fresh = ngram_tables_upload(e, host->d, V, host->start, &tables);
        }
        // searches already enqueued read the old tables: let them finish before the memory goes
        if (model->lodr_dev) {
            try {
                e.synchronize();
            } catch (...) {
                if (fresh) {
                    try { e.dev_free(fresh); } catch (...) {}
                }
                throw;
            }
        }
        e.set_lodr_tables(tables);
        model->lodr_serial = fresh ? ++g_hw_serial : 0;
        model->lodr_lm = std::move(copy);
        model->lodr_host = std::move(host);
        void* old = model->lodr_dev;
        model->lodr_dev = fresh;
        if (old) e.dev_free(old);
    });
}
int32_t k2hip_ctc_greedy(k2hip_model_t* model, const float* log_probs, int32_t B, int32_t Tprime, const int32_t* frame_offsets,
                         int64_t* tokens, int32_t* timestamps, int32_t* n_tokens, int32_t max_tokens, int32_t* num_trailing_blank) {
    return guard([&] {
        NEED(model); NEED(log_probs); NEED(tokens); NEED(timestamps); NEED(n_tokens);
        Engine& e = model->engine;
        K2_REQUIRE(e.model().cfg().ctc, "ctc_greedy: model_type '%s' has no CTC head", e.model().cfg().model_type.c_str());
        EngineLock lk(e);
        e.greedy_host(log_probs, B, Tprime, false, tokens, timestamps, n_tokens, max_tokens);
        for (int b = 0; b < B; b++) {
            if (frame_offsets)
                for (int k = 0; k < n_tokens[b]; k++) timestamps[(size_t)b * max_tokens + k] += frame_offsets[b];
            if (num_trailing_blank) num_trailing_blank[b] = e.last_any()[b] ? e.last_trail()[b] : num_trailing_blank[b] + e.last_trail()[b];
        }
    });
}
int32_t k2hip_offline_stream_get_ctc_state(const k2hip_offline_stream_t* s, int32_t* frame_offset, int32_t* num_trailing_blank) {
    return guard([&] {
        NEED(s);
        if (frame_offset) *frame_offset = s->frame_offset;
        if (num_trailing_blank) *num_trailing_blank = s->num_trailing_blank;
    });
}
int32_t k2hip_set_decoding_method(k2hip_model_t* model, const char* method, int32_t beam) {
    return guard([&] {
        NEED(model); NEED(method);
        Engine& e = model->engine;
        EngineLock lk(e);
        // leaving ctc_prefix_beam_search: a CTC model's other searches have no alternatives, so the N-best setting goes back to 1
        auto leave_prefix = [&] {
            if (e.ctc_prefix() == 0) return;
            K2_REQUIRE(e.batches_in_flight() == 0, "set_decoding_method: %d submitted batches are in flight; wait for them first", e.batches_in_flight());
            e.set_ctc_prefix(0);
            e.set_nbest(0);
            model->nbest = 1;
        };
        if (!strcmp(method, "greedy_search")) {
            leave_prefix();
            e.set_beam(0);
        } else if (!strcmp(method, "modified_beam_search")) {
            K2_REQUIRE(beam >= 1 && beam <= kMaxBeam, "modified_beam_search: beam %d out of range [1,%d]", beam, kMaxBeam);
            leave_prefix();
            e.set_beam(beam);
        } else if (!strcmp(method, "ctc_prefix_beam_search")) {
            if (!e.model().cfg().ctc)
                failf(K2HIP_ERR_UNSUPPORTED, "ctc_prefix_beam_search: model_type '%s' has no CTC head", e.model().cfg().model_type.c_str());
            K2_REQUIRE(beam >= 1 && beam <= kMaxBeam, "ctc_prefix_beam_search: beam %d out of range [1,%d]", beam, kMaxBeam);
            K2_REQUIRE(e.nbest() <= beam, "ctc_prefix_beam_search: the model keeps %d alternatives (k2hip_set_nbest), more than beam %d", e.nbest(), beam);
            e.set_ctc_prefix(beam);
        } else {
            failf(K2HIP_ERR_UNSUPPORTED, "decoding method '%s' (have: greedy_search, modified_beam_search, ctc_prefix_beam_search)", method);
        }
    });
}
int32_t k2hip_beam_search(k2hip_model_t* model, const float* enc_out, int32_t B, int32_t Tprime, int32_t beam, int64_t* tokens,
                          int32_t* timestamps, int32_t* n_tokens, int32_t max_tokens, float* scores) {
    return guard([&] {
        NEED(model); NEED(enc_out); NEED(tokens); NEED(timestamps); NEED(n_tokens);
        K2_REQUIRE(beam >= 1 && beam <= kMaxBeam, "beam search: beam %d out of range [1,%d]", beam, kMaxBeam);
        Engine& e = model->engine;
        EngineLock lk(e);
        struct Restore {
            Engine& e; int old;
            ~Restore() { e.set_beam(old); }
        } restore{e, e.beam()};
        e.set_beam(beam);
        e.greedy_host(enc_out, B, Tprime, false, tokens, timestamps, n_tokens, max_tokens);
        if (scores) memcpy(scores, e.last_scores().data(), sizeof(float) * B);
    });
}
int32_t k2hip_last_scores(k2hip_model_t* model, float* scores, int32_t B) {
    return guard([&] {
        NEED(model); NEED(scores);
        EngineLock lk(model->engine);
        K2_REQUIRE((size_t)B == model->engine.last_scores().size(), "last_scores: the last beam-search call had %zu streams, not %d",
                   model->engine.last_scores().size(), B);
        memcpy(scores, model->engine.last_scores().data(), sizeof(float) * B);
    });
}
int32_t k2hip_set_nbest(k2hip_model_t* model, int32_t n) {
    return guard([&] {
        NEED(model);
        K2_REQUIRE(n >= 1 && n <= kMaxBeam, "set_nbest: n = %d out of range [1,%d]", n, kMaxBeam);
        Engine& e = model->engine;
        EngineLock lk(e);
        if (n > 1 && e.model().cfg().ctc && e.ctc_prefix() == 0)
            failf(K2HIP_ERR_UNSUPPORTED, "set_nbest: a CTC model has no beam search to take alternatives from (ctc_prefix_beam_search has: "
                                         "k2hip_set_decoding_method first)");
        K2_REQUIRE(e.ctc_prefix() == 0 || n <= e.ctc_prefix(), "set_nbest: n = %d above the prefix search's beam %d", n, e.ctc_prefix());
        K2_REQUIRE(n == 1 || e.beam() > 0 || e.ctc_prefix() > 0, "set_nbest: alternatives come from modified_beam_search; the model decodes with greedy_search "
                                           "(k2hip_set_decoding_method first)");
        K2_REQUIRE(e.batches_in_flight() == 0, "set_nbest: %d submitted batches are in flight; wait for them first", e.batches_in_flight());
        e.set_nbest(n > 1 ? n : 0);
        model->nbest = n;
    });
}
// the alternatives of a stream (empty list: the start state) through the getters' common rules
static void alt_get(const std::vector<BeamAlt>& alts, int32_t i, int64_t* tokens, int32_t* timestamps, float* token_log_probs, int32_t cap,
                    int32_t* n, float* score) {
    K2_REQUIRE(i >= 0 && i < (int32_t)alts.size(), "alternative %d of %zu", i, alts.size());
    const BeamAlt& a = alts[(size_t)i];
    if ((int64_t)a.tokens.size() > cap) failf(K2HIP_ERR_CAPACITY, "alternative %d holds %zu tokens", i, a.tokens.size());
    if (!a.tokens.empty()) {
        if (tokens) memcpy(tokens, a.tokens.data(), sizeof(int64_t) * a.tokens.size());
        if (timestamps) memcpy(timestamps, a.timestamps.data(), sizeof(int32_t) * a.timestamps.size());
        if (token_log_probs) memcpy(token_log_probs, a.token_log_probs.data(), sizeof(float) * a.token_log_probs.size());
    }
    if (n) *n = (int32_t)a.tokens.size();
    if (score) *score = a.score;
}
static int32_t yp_get(const std::vector<float>& yp, float* out, int32_t cap) {
    int32_t count = 0;
    const int32_t rc = guard([&] {
        if ((int64_t)yp.size() > cap) failf(K2HIP_ERR_CAPACITY, "the result holds %zu token log-probs", yp.size());
        if (!yp.empty()) {
            NEED(out);
            memcpy(out, yp.data(), sizeof(float) * yp.size());
        }
        count = (int32_t)yp.size();
    });
    return rc < 0 ? rc : count;
}
// entry (b, i) of the engine's last N-best as a BeamAlt
// Neural LM rescoring of the streams' N-best lists (k2hip.h "Neural LM rescoring"): all alternatives of all streams through ONE scoring
// call with_eos, each list stably re-ordered by the method's own ordering quantity over score + scale * lm_total, entry 0 written
// into the call's result rows.  Under the engine's lock.
static void rnn_lm_rescore(k2hip_model* model, k2hip_offline_stream_t* const* streams, int B, int max_tokens, int64_t* tok, int32_t* ts, int32_t* n) {
    Engine& e = model->engine;
    const bool ctc = e.model().cfg().ctc;
    std::vector<int64_t> ids, off(1, 0);
    for (int b = 0; b < B; b++)
        for (const BeamAlt& a : streams[b]->alts) {
            ids.insert(ids.end(), a.tokens.begin(), a.tokens.end());
            off.push_back((int64_t)ids.size());
        }
    const int Hn = (int)off.size() - 1;
    if (Hn == 0) return;
    std::vector<float> totals((size_t)Hn);
    e.rnn_lm_score_host(ids.data(), off.data(), Hn, true, nullptr, totals.data());
    const float scale = model->rnn_scale;
    // LODR: lodr_i on the host, the model's scaled automaton walked over the alternative's tokens (a list is at most 8 short hypotheses)
    const LodrHost* lodr = model->lodr_host.get();
    int at = 0;
    for (int b = 0; b < B; b++) {
        std::vector<BeamAlt>& alts = streams[b]->alts;
        const size_t N = alts.size();
        std::vector<float> key(N);
        for (size_t i = 0; i < N; i++) {
            alts[i].lm_score = totals[(size_t)at++];
            volatile float term = scale * alts[i].lm_score;   // (the product rounded to float32, then the sum: no contraction)
            volatile float sum = alts[i].score + term;
            if (lodr) {   // (score_i + fl32(scale lm_i)) + lodr_i
                alts[i].lodr_score = lodr->total(alts[i].tokens.data(), alts[i].tokens.size());
                sum = sum + alts[i].lodr_score;
            }
            key[i] = ctc ? sum : sum / (float)(alts[i].tokens.size() + 2);
        }
        std::vector<size_t> ord(N);
        for (size_t i = 0; i < N; i++) ord[i] = i;
        std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return key[x] > key[y]; });
        std::vector<BeamAlt> sorted;
        sorted.reserve(N);
        for (size_t i = 0; i < N; i++) sorted.push_back(std::move(alts[ord[i]]));
        alts.swap(sorted);
        if (alts.empty()) continue;
        const BeamAlt& best = alts[0];
        K2_REQUIRE((int64_t)best.tokens.size() <= max_tokens, "internal: a rescored alternative of stream %d holds %zu tokens, the result row %d", b,
                   best.tokens.size(), max_tokens);
        n[b] = (int32_t)best.tokens.size();
        for (size_t k = 0; k < best.tokens.size(); k++) {
            tok[(size_t)b * max_tokens + k] = best.tokens[k];
            ts[(size_t)b * max_tokens + k] = best.timestamps[k];
        }
    }
}
static BeamAlt alt_of(const Engine::NbestHost& h, int b, int i) {
    BeamAlt a;
    const size_t e = (size_t)b * h.N + i, o = e * h.max_tokens, len = (size_t)h.n_tokens[e];
    a.tokens.assign(h.tokens.begin() + o, h.tokens.begin() + o + len);
    a.timestamps.assign(h.timestamps.begin() + o, h.timestamps.begin() + o + len);
    a.token_log_probs.assign(h.token_log_probs.begin() + o, h.token_log_probs.begin() + o + len);
    a.score = h.scores[e];
    return a;
}
int32_t k2hip_beam_search_nbest(k2hip_model_t* model, const float* enc_out, int32_t B, int32_t Tprime, int32_t beam, int32_t nbest,
                                int64_t* tokens, int32_t* timestamps, float* token_log_probs, int32_t* n_tokens, int32_t* n_hyps, float* scores,
                                int32_t max_tokens) {
    return guard([&] {
        NEED(model); NEED(enc_out); NEED(tokens); NEED(timestamps); NEED(token_log_probs); NEED(n_tokens); NEED(n_hyps); NEED(scores);
        K2_REQUIRE(beam >= 1 && beam <= kMaxBeam, "beam search: beam %d out of range [1,%d]", beam, kMaxBeam);
        K2_REQUIRE(nbest >= 1 && nbest <= kMaxBeam, "beam search: nbest %d out of range [1,%d]", nbest, kMaxBeam);
        K2_REQUIRE(B > 0 && Tprime > 0 && max_tokens > 0, "beam search: bad shape B=%d T'=%d max_tokens=%d", B, Tprime, max_tokens);
        Engine& e = model->engine;
        if (e.model().cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "beam search: a CTC model has no transducer search");
        EngineLock lk(e);
        struct Restore {
            Engine& e; int beam, nbest;
            ~Restore() { e.set_beam(beam); e.set_nbest(nbest); }
        } restore{e, e.beam(), e.nbest()};
        e.set_beam(beam);
        e.set_nbest(nbest);
        // (the single result goes to scratch: entry 0 of the list is that result)
        std::vector<int64_t> tok1((size_t)B * max_tokens);
        std::vector<int32_t> ts1((size_t)B * max_tokens), n1((size_t)B);
        e.greedy_host(enc_out, B, Tprime, false, tok1.data(), ts1.data(), n1.data(), max_tokens);
        const Engine::NbestHost& h = e.last_nbest();
        K2_REQUIRE(h.B == B && h.N == nbest && h.max_tokens == max_tokens, "internal: the search kept no N-best");
        for (int b = 0; b < B; b++) {
            n_hyps[b] = h.n_hyps[(size_t)b];
            for (int i = 0; i < h.n_hyps[(size_t)b]; i++) {
                const size_t en = (size_t)b * nbest + i, o = en * max_tokens, len = (size_t)h.n_tokens[en];
                memcpy(tokens + o, h.tokens.data() + o, sizeof(int64_t) * len);
                memcpy(timestamps + o, h.timestamps.data() + o, sizeof(int32_t) * len);
                memcpy(token_log_probs + o, h.token_log_probs.data() + o, sizeof(float) * len);
                n_tokens[en] = (int32_t)len;
                scores[en] = h.scores[en];
            }
        }
    });
}
// CTC prefix beam search, operator level: the engine checks the arguments on the host before any device work (ctc_prefix_ref.h)
int32_t k2hip_ctc_prefix_beam_search(k2hip_model_t* model, const float* log_probs, int32_t R, int32_t Tprime, const int32_t* n_frames, int32_t beam,
                                     int32_t nbest, int64_t* tokens, int32_t* timestamps, float* token_log_probs, int32_t* n_tokens,
                                     int32_t* n_hyps, float* scores, int32_t max_tokens) {
    return guard([&] {
        NEED(model); NEED(log_probs); NEED(tokens); NEED(timestamps); NEED(token_log_probs); NEED(n_tokens); NEED(n_hyps); NEED(scores);
        Engine& e = model->engine;
        if (!e.model().cfg().ctc)
            failf(K2HIP_ERR_UNSUPPORTED, "ctc_prefix_beam_search: model_type '%s' has no CTC head", e.model().cfg().model_type.c_str());
        EngineLock lk(e);
        e.ctc_prefix_host(log_probs, R, Tprime, n_frames, beam, nbest, tokens, timestamps, token_log_probs, n_tokens, n_hyps, scores, max_tokens);
    });
}
// the opt-in of the offline prefix search's hotword / n-gram LM biasing (off: the tables on the model are ignored by that search)
int32_t k2hip_set_ctc_prefix_biasing(k2hip_model_t* model, int32_t on) {
    return guard([&] {
        NEED(model);
        Engine& e = model->engine;
        if (!e.model().cfg().ctc)
            failf(K2HIP_ERR_UNSUPPORTED, "set_ctc_prefix_biasing: model_type '%s' has no CTC head", e.model().cfg().model_type.c_str());
        EngineLock lk(e);
        K2_REQUIRE(e.batches_in_flight() == 0, "set_ctc_prefix_biasing: %d submitted batches are in flight; wait for them first", e.batches_in_flight());
        e.set_ctc_prefix_biasing(on != 0);
    });
}
// forced alignment / full-sum scoring: the engine checks the targets on the host before any device work (lattice_ref.h)
int32_t k2hip_transducer_align(k2hip_model_t* model, const float* enc_out, int32_t B, int32_t Tprime, const int32_t* n_frames,
                               const int64_t* ids, const int32_t* lens, int32_t* timestamps, float* token_log_probs, float* total_logp,
                               float* best_logp, int32_t max_tokens) {
    return guard([&] {
        NEED(model); NEED(enc_out); NEED(lens);
        K2_REQUIRE(B > 0 && Tprime > 0 && max_tokens >= 0, "align: bad shape B=%d T'=%d max_tokens=%d", B, Tprime, max_tokens);
        Engine& e = model->engine;
        if (e.model().cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "align: a CTC model has no transducer lattice");
        EngineLock lk(e);
        e.align_host(enc_out, B, Tprime, n_frames, ids, lens, timestamps, token_log_probs, total_logp, best_logp, max_tokens);
    });
}
int32_t k2hip_offline_align_from_samples(k2hip_model_t* model, const float* const* samples, const int64_t* n_samples, int32_t B,
                                         const int64_t* ids, const int32_t* lens, int32_t* timestamps, float* token_log_probs,
                                         float* total_logp, float* best_logp, int32_t max_tokens, int32_t* Tprime_out) {
    return guard([&] {
        NEED(model); NEED(samples); NEED(n_samples); NEED(lens);
        K2_REQUIRE(B > 0 && max_tokens >= 0, "align_from_samples: bad shape B=%d max_tokens=%d", B, max_tokens);
        Engine& e = model->engine;
        if (e.model().cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "align: a CTC model has no transducer lattice");
        EngineLock lk(e);
        e.align_samples(samples, n_samples, B, ids, lens, timestamps, token_log_probs, total_logp, best_logp, max_tokens, Tprime_out);
    });
}
// CTC forced alignment / full-sum scoring: the engine checks the targets on the host before any device work (ctc_lattice_ref.h)
int32_t k2hip_ctc_align(k2hip_model_t* model, const float* log_probs, int32_t R, int32_t Tprime, const int32_t* n_frames, int32_t H,
                        const int32_t* stream_of, const int64_t* ids, const int32_t* lens, int32_t* timestamps, int32_t* end_frames,
                        float* token_log_probs, float* total_logp, float* best_logp, int32_t max_tokens) {
    return guard([&] {
        NEED(model); NEED(log_probs); NEED(lens);
        K2_REQUIRE(R > 0 && Tprime > 0 && H > 0 && max_tokens >= 0, "ctc_align: bad shape R=%d T'=%d H=%d max_tokens=%d", R, Tprime, H, max_tokens);
        Engine& e = model->engine;
        if (!e.model().cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "ctc_align: model_type '%s' has no CTC head", e.model().cfg().model_type.c_str());
        EngineLock lk(e);
        e.ctc_align_host(log_probs, R, Tprime, n_frames, H, stream_of, ids, lens, timestamps, end_frames, token_log_probs, total_logp, best_logp,
                         max_tokens);
    });
}
int32_t k2hip_offline_ctc_align_from_samples(k2hip_model_t* model, const float* const* samples, const int64_t* n_samples, int32_t B, int32_t H,
                                             const int32_t* stream_of, const int64_t* ids, const int32_t* lens, int32_t* timestamps,
                                             int32_t* end_frames, float* token_log_probs, float* total_logp, float* best_logp,
                                             int32_t max_tokens, int32_t* Tprime_out) {
    return guard([&] {
        NEED(model); NEED(samples); NEED(n_samples); NEED(lens);
        K2_REQUIRE(B > 0 && H > 0 && max_tokens >= 0, "ctc_align_from_samples: bad shape B=%d H=%d max_tokens=%d", B, H, max_tokens);
        Engine& e = model->engine;
        if (!e.model().cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "ctc_align: model_type '%s' has no CTC head", e.model().cfg().model_type.c_str());
        EngineLock lk(e);
        e.ctc_align_samples(samples, n_samples, B, H, stream_of, ids, lens, timestamps, end_frames, token_log_probs, total_logp, best_logp,
                            max_tokens, Tprime_out);
    });
}
int32_t k2hip_offline_greedy(k2hip_model_t* model, const float* const* feats, const int64_t* n_floats, int32_t B,
                             int64_t* tokens, int32_t* timestamps, int32_t* n_tokens, int32_t max_tokens) {
    return guard([&] {
        NEED(model); NEED(feats); NEED(n_floats); NEED(tokens); NEED(timestamps); NEED(n_tokens);
        EngineLock lk(model->engine);
        model->engine.offline_greedy_feats(feats, n_floats, B, false, tokens, timestamps, n_tokens, max_tokens);
    });
}
int32_t k2hip_offline_greedy_single(k2hip_model_t* model, const float* feats, int64_t n_floats, int64_t* tokens,
                                    int32_t* timestamps, int32_t* n_tokens, int32_t max_tokens) {
    return guard([&] {
        NEED(model); NEED(feats); NEED(tokens); NEED(timestamps); NEED(n_tokens);
        EngineLock lk(model->engine);
        const float* p[1] = {feats};
        int64_t n[1] = {n_floats};
        model->engine.offline_greedy_feats(p, n, 1, true, tokens, timestamps, n_tokens, max_tokens);
    });
}
int32_t k2hip_offline_greedy_from_samples(k2hip_model_t* model, const float* const* samples, const int64_t* n_samples,
                                          int32_t B, int64_t* tokens, int32_t* timestamps, int32_t* n_tokens,
                                          int32_t max_tokens) {
    return guard([&] {
        NEED(model); NEED(samples); NEED(n_samples); NEED(tokens); NEED(timestamps); NEED(n_tokens);
        EngineLock lk(model->engine);
        model->engine.offline_greedy_samples(samples, n_samples, B, tokens, timestamps, n_tokens, max_tokens);
    });
}
int32_t k2hip_offline_greedy_from_samples_dev(k2hip_model_t* model, const float* samples_dev, int64_t n_samples_each,
                                              int32_t B, int64_t* tokens, int32_t* timestamps, int32_t* n_tokens,
                                              int32_t max_tokens) {
    return guard([&] {
        NEED(model); NEED(samples_dev); NEED(tokens); NEED(timestamps); NEED(n_tokens);
        EngineLock lk(model->engine);
        model->engine.offline_greedy_samples_dev(samples_dev, n_samples_each, B, tokens, timestamps, n_tokens, max_tokens);
    });
}

int32_t k2hip_offline_submit_samples_dev(k2hip_model_t* model, const float* samples_dev, int64_t n_samples_each, int32_t B,
                                         int32_t max_tokens, int32_t* ticket) {
    return guard([&] {
        NEED(model); NEED(samples_dev); NEED(ticket);
        EngineLock lk(model->engine);
        K2_REQUIRE(model->engine.nbest() == 0, "offline submit: the pipelined route returns one result per stream and the model keeps %d "
                   "alternatives (k2hip_set_nbest) -- use the synchronous entries, or set_nbest(model, 1)", model->engine.nbest());
        *ticket = model->engine.submit_samples_dev(samples_dev, n_samples_each, B, max_tokens);
    });
}
int32_t k2hip_offline_submit_samples(k2hip_model_t* model, const float* samples_host, int64_t n_samples_each, int32_t B,
                                     int32_t max_tokens, int32_t* ticket) {
    return guard([&] {
        NEED(model); NEED(samples_host); NEED(ticket);
        EngineLock lk(model->engine);
        K2_REQUIRE(model->engine.nbest() == 0, "offline submit: the pipelined route returns one result per stream and the model keeps %d "
                   "alternatives (k2hip_set_nbest) -- use the synchronous entries, or set_nbest(model, 1)", model->engine.nbest());
        *ticket = model->engine.submit_samples_host(samples_host, n_samples_each, B, max_tokens);
    });
}
int32_t k2hip_host_alloc(k2hip_model_t* model, int64_t bytes, void** host_ptr) {
    return guard([&] {
        NEED(model); NEED(host_ptr);
        K2_REQUIRE(bytes > 0, "host_alloc: %lld bytes", (long long)bytes);
        *host_ptr = model->engine.host_alloc(bytes);
    });
}
int32_t k2hip_host_free(k2hip_model_t* model, void* host_ptr) {
    return guard([&] {
        NEED(model);
        if (host_ptr) model->engine.host_free(host_ptr);
    });
}
int32_t k2hip_offline_wait(k2hip_model_t* model, int32_t ticket, int64_t* tokens, int32_t* timestamps, int32_t* n_tokens) {
    return guard([&] {
        NEED(model); NEED(tokens); NEED(timestamps); NEED(n_tokens);
        EngineLock lk(model->engine);
        K2_REQUIRE(model->engine.nbest() == 0, "offline wait: the pipelined route returns one result per stream and the model keeps %d "
                   "alternatives (k2hip_set_nbest)", model->engine.nbest());
        model->engine.wait_ticket(ticket, tokens, timestamps, n_tokens);
    });
}

int32_t k2hip_device_alloc(k2hip_model_t* model, int64_t bytes, void** dev_ptr) {
    return guard([&] {
        NEED(model); NEED(dev_ptr);
        *dev_ptr = model->engine.dev_alloc(bytes);
    });
}
int32_t k2hip_device_free(k2hip_model_t* model, void* dev_ptr) {
    return guard([&] {
        NEED(model);
        if (dev_ptr) model->engine.dev_free(dev_ptr);
    });
}
int32_t k2hip_device_upload(k2hip_model_t* model, void* dev_dst, const void* host_src, int64_t bytes) {
    return guard([&] {
        NEED(model); NEED(dev_dst); NEED(host_src);
        model->engine.dev_upload(dev_dst, host_src, bytes);
    });
}
int32_t k2hip_synchronize(k2hip_model_t* model) {
    return guard([&] {
        NEED(model);
        model->engine.synchronize();
    });
}

// ---- OnlineStream / OnlineRecognizer ----------------------------------------------------------
int32_t k2hip_online_stream_create(k2hip_model_t* model, k2hip_online_stream_t** out) {
    return guard([&] {
        NEED(model); NEED(out);
        *out = nullptr;
        EngineLock lk(model->engine);
        auto* s = new k2hip_online_stream();
        s->model = model;
        try {
            s->slot = model->engine.online_alloc_slot();
        } catch (...) {
            delete s;
            throw;
        }
        // OnlineProjOfConformer.GetEncoderInitStates (:76-77) starts processed_lens at 2, not 0
        if (model->engine.model().cfg().conformer) s->processed_len = 2;
        *out = s;
    });
}
// Back to the state of a freshly created stream (new utterance on the same object): caches zeroed in place, FIFOs, tokens,
// timestamps and Hyp cleared.  The reference has no such method -- a host would drop the OnlineStream and create a new one
// (OnlineRecognizer.cs:60-64); this keeps the slot and skips the allocation.
int32_t k2hip_online_stream_reset(k2hip_online_stream_t* s) {
    return guard([&] {
        NEED(s);
        k2hip_model* model = s->model;
        {
            EngineLock lk(model->engine);
            model->engine.online_free_slot(s->slot);
            s->slot = -1;
            s->slot = model->engine.online_alloc_slot();  // (the slot just freed: re-zeroed like GetEncoderInitStates)
        }
        std::shared_ptr<HwResident> hw = std::move(s->hw);   // (the attached hotword graph stays; every hypothesis is back at its root)
        const int cp_beam = s->cp_beam, cp_nbest = s->cp_nbest;   // (so does the prefix-search setting; its prefixes go)
        const bool cp_biasing = s->cp_biasing;
        *s = k2hip_online_stream{model, s->slot};
        s->hw = std::move(hw);
        s->cp_biasing = cp_biasing;
        s->cp_beam = cp_beam;
        s->cp_nbest = cp_nbest;
        if (model->engine.model().cfg().conformer) s->processed_len = 2;
    });
}
int32_t k2hip_online_stream_set_hotwords(k2hip_online_stream_t* s, const k2hip_hotwords_t* hw) {
    return guard([&] {
        NEED(s);
        K2_REQUIRE(s->chunks_done == 0 && s->method < 0, "online stream set_hotwords: the stream has decoded %lld chunks and its hypotheses carry "
                   "states of the graph it started with -- reset the stream first", s->chunks_done);
        s->hw = hw ? hw_resident_get(s->model, hw, "online stream set_hotwords") : nullptr;
        if (s->beam) s->beam->set_pending(s->hw ? s->hw->pending : nullptr);
    });
}
int32_t k2hip_online_stream_set_ctc_prefix_beam(k2hip_online_stream_t* s, int32_t beam, int32_t nbest) {
    return guard([&] {
        NEED(s);
        const Config& c = s->model->engine.model().cfg();
        if (!c.ctc) failf(K2HIP_ERR_UNSUPPORTED, "online stream set_ctc_prefix_beam: model_type '%s' has no CTC head", c.model_type.c_str());
        K2_REQUIRE(beam >= 0 && beam <= kMaxBeam, "online stream set_ctc_prefix_beam: beam %d out of range [0 = off, 1..%d]", beam, kMaxBeam);
        K2_REQUIRE(beam == 0 || (nbest >= 1 && nbest <= beam), "online stream set_ctc_prefix_beam: nbest %d out of range [1, beam = %d]", nbest, beam);
        K2_REQUIRE(s->chunks_done == 0 && s->method < 0, "online stream set_ctc_prefix_beam: the stream has searched %lld chunks and its result "
                   "belongs to the search it started with -- reset the stream first", s->chunks_done);
        s->cp_beam = beam;
        s->cp_nbest = beam ? nbest : 1;
        s->cprefix.reset();
    });
}
int32_t k2hip_online_stream_set_ctc_prefix_biasing(k2hip_online_stream_t* s, int32_t on) {
    return guard([&] {
        NEED(s);
        const Config& c = s->model->engine.model().cfg();
        if (!c.ctc) failf(K2HIP_ERR_UNSUPPORTED, "online stream set_ctc_prefix_biasing: model_type '%s' has no CTC head", c.model_type.c_str());
        K2_REQUIRE(s->chunks_done == 0 && s->method < 0, "online stream set_ctc_prefix_biasing: the stream has searched %lld chunks and its prefixes "
                   "carry the states of the search it started with -- reset the stream first", s->chunks_done);
        s->cp_biasing = on != 0;
    });
}
int32_t k2hip_online_stream_destroy(k2hip_online_stream_t* s) {
    return guard([&] {
        if (!s) return;
        {
            EngineLock lk(s->model->engine);
            s->model->engine.online_free_slot(s->slot);
        }
        delete s;
    });
}
int32_t k2hip_online_chunk_info(const k2hip_model_t* model, int32_t* chunk_length, int32_t* shift_length, int32_t* frames_per_chunk) {
    return guard([&] {
        NEED(model);
        const Config& c = model->engine.model().cfg();
        K2_REQUIRE(c.streaming || c.lstm, "this model is not a streaming export");
        if (chunk_length) *chunk_length = c.chunk_T;
        if (shift_length) *shift_length = c.shift;
        if (frames_per_chunk) *frames_per_chunk = model->engine.online_frames_per_chunk();
    });
}
// the model's plan for input at `rate` (null: the model's own rate); built once per rate
static const ResamplePlan* model_resample_plan(k2hip_model* m, int rate) {
    const int out = m->engine.model().cfg().fbank.sample_rate;
    K2_REQUIRE(rate > 0, "sample rate %d", rate);
    if (rate == out) return nullptr;
    std::lock_guard<std::mutex> lk(m->rs_mu);
    auto it = m->rs_plans.find(rate);
    if (it == m->rs_plans.end()) it = m->rs_plans.emplace(rate, std::make_unique<ResamplePlan>(resample_plan(rate, out))).first;
    return it->second.get();
}
constexpr int64_t kResampleMaxInput = (int64_t)1 << 36;   // input samples of one stream: keeps the plan's tick arithmetic inside int64
// the rule of the accept_waveform entries, offline and online: a stream's rate (*s_rate, 0 = none yet) and plan (*s_rs) are fixed by
// its first samples; returns the plan
static const ResamplePlan* take_rate(k2hip_model* m, int* s_rate, const ResamplePlan** s_rs, int rate, const char* who) {
    if (*s_rate == 0) {
        const ResamplePlan* p = model_resample_plan(m, rate);   // (a refused plan leaves the stream without a rate)
        *s_rate = rate;
        *s_rs = p;
    }
    K2_REQUIRE(*s_rate == rate, "%s: the stream takes samples at %d Hz, these are at %d Hz", who, *s_rate, rate);
    return *s_rs;
}
static void online_add_samples(k2hip_online_stream* s, const float* samples, int64_t n) {
    if (n <= 0) return;
    const int own = s->model->engine.model().cfg().fbank.sample_rate;
    K2_REQUIRE(!s->rs, "accept_samples: the stream resamples from %d Hz (accept_waveform), these samples are at the model's %d Hz", s->rate, own);
    s->rate = own;
    s->pending.insert(s->pending.end(), samples, samples + n);  // OnlineStream.AddSamples (:57-79), fbank deferred
}
static void online_add_waveform(k2hip_online_stream* s, int rate, const float* samples, int64_t n) {
    if (!take_rate(s->model, &s->rate, &s->rs, rate, "accept_waveform")) return online_add_samples(s, samples, n);
    if (n <= 0) return;
    K2_REQUIRE(s->rs_n_in + (int64_t)s->rs_in.size() + n < kResampleMaxInput, "accept_waveform: more than 2^36 samples in one stream");
    s->rs_in.insert(s->rs_in.end(), samples, samples + n);
}
// samples at the model's rate that the stream's queued input will give
static int64_t online_resample_due(const k2hip_online_stream* s) {
    return s->rs ? s->rs->num_out(s->rs_n_in + (int64_t)s->rs_in.size()) - s->rs_n_out : 0;
}
// frames the stream's pending samples will add to Speech
static int64_t online_pending_frames(const k2hip_online_stream* s) {
    const int64_t due = online_resample_due(s);
    return s->pending.empty() && due == 0 ? 0 : s->model->engine.fbank_num_frames((int64_t)(s->remainder.size() + s->pending.size()) + due);
}
// the queued input of every resampling stream among `streams` through the resampler, ONE launch across their rates; the outputs join
// `pending`, the streams keep the input tail that later outputs read
static void online_resample(k2hip_online_stream* const* streams, int n) {
    std::vector<k2hip_online_stream*> g;
    for (int i = 0; i < n; i++)
        if (streams[i]->rs && !streams[i]->rs_in.empty()) g.push_back(streams[i]);
    if (g.empty()) return;
    std::vector<std::vector<float>> out(g.size());
    std::vector<Engine::ResampleJob> jobs;
    for (size_t i = 0; i < g.size(); i++) {
        k2hip_online_stream* s = g[i];
        out[i].resize((size_t)online_resample_due(s));
        if (out[i].empty()) continue;   // (a push that completes no output: bookkeeping only)
        jobs.push_back(Engine::ResampleJob{s->rs, s->rs_tail.data(), (int64_t)s->rs_tail.size(), s->rs_in.data(), (int64_t)s->rs_in.size(),
                                           s->rs_n_in - (int64_t)s->rs_tail.size(), s->rs_n_out, (int64_t)out[i].size(), out[i].data()});
    }
    if (!jobs.empty()) {
        Engine& e = g[0]->model->engine;
        EngineLock lk(e);
        e.resample_host(jobs.data(), (int)jobs.size());
    }
    for (size_t i = 0; i < g.size(); i++) {
        k2hip_online_stream* s = g[i];
        const int64_t x0 = s->rs_n_in - (int64_t)s->rs_tail.size();
        s->rs_n_in += (int64_t)s->rs_in.size();
        s->rs_n_out += (int64_t)out[i].size();
        const int64_t keep = std::min(s->rs->keep_from(s->rs_n_out), s->rs_n_in);
        s->rs_tail.insert(s->rs_tail.end(), s->rs_in.begin(), s->rs_in.end());
        s->rs_tail.erase(s->rs_tail.begin(), s->rs_tail.begin() + (keep - x0));
        s->rs_in.clear();
        s->pending.insert(s->pending.end(), out[i].begin(), out[i].end());
    }
}
static int64_t online_logical_floats(const k2hip_online_stream* s) {
    return (int64_t)s->speech.size() + online_pending_frames(s) * s->model->engine.model().cfg().feat;
}
// run the deferred fbank of `n` streams of one model: streams at the same position share one batched launch
// may_defer: the caller runs a chunk step on the same engine next and collects the frames after it (Engine::fbank_gather_finish);
// taken only when ONE batched launch covers every stream with queued samples.  Returns whether a gather was left outstanding.
static bool online_materialize(k2hip_online_stream* const* streams, int n, bool may_defer = false) {
    if (n <= 0) return false;
    online_resample(streams, n);
    bool deferred = false;
    Engine& e = streams[0]->model->engine;
    const Config& c = e.model().cfg();
    std::map<int64_t, std::vector<k2hip_online_stream*>> groups;  // by length of [remainder ; pending]
    for (int i = 0; i < n; i++) {
        k2hip_online_stream* s = streams[i];
        if (s->pending.empty()) continue;
        groups[(int64_t)(s->remainder.size() + s->pending.size())].push_back(s);
    }
    for (auto& kv : groups) {
        const int64_t len = kv.first, nf = e.fbank_num_frames(len);
        std::vector<k2hip_online_stream*>& g = kv.second;
        const int G = (int)g.size();
        if (nf == 0) {  // OnlineStream.cs:67: nothing is appended until the fbank produces a frame
            for (k2hip_online_stream* s : g) {
                s->remainder.insert(s->remainder.end(), s->pending.begin(), s->pending.end());
                s->pending.clear();
            }
            continue;
        }
        // [remainder ; pending] of every stream goes straight into the engine's pinned staging buffer, the frames come straight
        // out of it into the streams' Speech
        std::vector<const float*> hp(G), tp(G);
        std::vector<int64_t> hn(G), tn(G);
        std::vector<float*> dst(G);
        std::vector<int> fslot(G), fpos(G);
        for (int i = 0; i < G; i++) {
            k2hip_online_stream* s = g[i];
            hp[i] = s->remainder.data(); hn[i] = (int64_t)s->remainder.size();
            tp[i] = s->pending.data(); tn[i] = (int64_t)s->pending.size();
            const size_t old = s->speech.size();
            const int64_t have = (int64_t)(old / (size_t)c.feat);
            if (s->mir_ok && have + nf > Engine::kFifoFrames) s->mir_ok = false;  // the FIFO outgrows its device mirror
            fslot[i] = s->slot;
            fpos[i] = s->mir_ok ? (int)((s->mir_head + have) % Engine::kFifoFrames) : -1;
            s->speech.resize(old + (size_t)nf * c.feat);
            dst[i] = s->speech.data() + old;
        }
        try {
            EngineLock lk(e);
            const bool defer = may_defer && groups.size() == 1;
            e.fbank_host_gather(hp.data(), hn.data(), tp.data(), tn.data(), len, G, dst.data(), nf, fslot.data(), fpos.data(), defer);
            deferred = defer;
        } catch (...) {
            for (k2hip_online_stream* s : g) s->speech.resize(s->speech.size() - (size_t)nf * c.feat);  // nothing was appended
            throw;
        }
        const int64_t used = nf * c.fbank.frame_shift;  // samples consumed by whole frame shifts
        for (int i = 0; i < G; i++) {
            k2hip_online_stream* s = g[i];
            std::vector<float> rem((size_t)(len - used));
            // the new remainder is the tail of [remainder ; pending]
            for (int64_t k = used; k < len; k++) rem[(size_t)(k - used)] = k < hn[i] ? s->remainder[(size_t)k] : s->pending[(size_t)(k - hn[i])];
            s->remainder.swap(rem);
            s->pending.clear();
        }
    }
    return deferred;
}
int32_t k2hip_online_stream_accept_samples(k2hip_online_stream_t* s, const float* samples, int64_t n) {
    return guard([&] {
        NEED(s);
        if (n > 0) NEED(samples);
        online_add_samples(s, samples, n);
    });
}
int32_t k2hip_online_accept_samples_batch(k2hip_model_t* model, k2hip_online_stream_t* const* streams, int32_t B,
                                          const float* const* samples, const int64_t* n) {
    return guard([&] {
        NEED(model); NEED(streams); NEED(samples); NEED(n);
        K2_REQUIRE(B > 0, "accept_samples_batch: empty list");
        for (int i = 0; i < B; i++) {
            NEED(streams[i]);
            if (n[i] > 0) NEED(samples[i]);
            online_add_samples(streams[i], samples[i], n[i]);
        }
    });
}
int32_t k2hip_online_stream_accept_waveform(k2hip_online_stream_t* s, int32_t sample_rate, const float* samples, int64_t n) {
    return guard([&] {
        NEED(s);
        if (n > 0) NEED(samples);
        online_add_waveform(s, sample_rate, samples, n);
    });
}
int32_t k2hip_online_accept_waveform_batch(k2hip_model_t* model, k2hip_online_stream_t* const* streams, int32_t B, int32_t sample_rate,
                                           const float* const* samples, const int64_t* n) {
    return guard([&] {
        NEED(model); NEED(streams); NEED(samples); NEED(n);
        K2_REQUIRE(B > 0, "accept_waveform_batch: empty list");
        const int own = model->engine.model().cfg().fbank.sample_rate;
        model_resample_plan(model, sample_rate);   // (a rate that is refused is refused before any stream takes a sample)
        for (int i = 0; i < B; i++) {
            NEED(streams[i]);
            if (n[i] > 0) NEED(samples[i]);
            K2_REQUIRE(streams[i]->model == model, "accept_waveform_batch: stream %d belongs to another model", i);
            K2_REQUIRE(streams[i]->rate == 0 || streams[i]->rate == sample_rate, "accept_waveform_batch: stream %d takes samples at %d Hz, these are at "
                       "%d Hz (the model's: %d Hz)", i, streams[i]->rate, sample_rate, own);
        }
        for (int i = 0; i < B; i++) online_add_waveform(streams[i], sample_rate, samples[i], n[i]);
    });
}
// ---- the resampler alone (include/k2hip.h "Input at other sample rates") ----
int64_t k2hip_resample_num_out(k2hip_model_t* model, int32_t in_rate, int64_t n_in_total) {
    int64_t r = -1;
    guard([&] {
        NEED(model);
        K2_REQUIRE(n_in_total >= 0 && n_in_total < kResampleMaxInput, "resample_num_out: %lld samples", (long long)n_in_total);
        const ResamplePlan* p = model_resample_plan(model, in_rate);
        r = p ? p->num_out(n_in_total) : n_in_total;
    });
    return r;
}
int32_t k2hip_resample(k2hip_model_t* model, int32_t in_rate, const float* samples, int64_t n, float* out, int64_t cap, int64_t* n_out) {
    return guard([&] {
        NEED(model); NEED(n_out);
        K2_REQUIRE(n >= 0 && n < kResampleMaxInput && cap >= 0, "resample: %lld samples into %lld", (long long)n, (long long)cap);
        if (n > 0) NEED(samples);
        const ResamplePlan* p = model_resample_plan(model, in_rate);
        const int64_t no = p ? p->num_out(n) : n;
        *n_out = no;
        if (no > cap) failf(K2HIP_ERR_CAPACITY, "resample: %lld samples at %d Hz give %lld, capacity %lld", (long long)n, in_rate, (long long)no, (long long)cap);
        if (no == 0) return;
        NEED(out);
        if (!p) {
            memcpy(out, samples, sizeof(float) * (size_t)n);
            return;
        }
        const Engine::ResampleJob job{p, samples, n, nullptr, 0, 0, 0, no, out};
        EngineLock lk(model->engine);
        model->engine.resample_host(&job, 1);
    });
}
// test hooks (include/k2hip_debug.h): the plan and the float32 host reference, no model and no GPU
int32_t k2hip_debug_resample_plan(int32_t in_rate, int32_t out_rate, int32_t* iu, int32_t* ou, int32_t* max_taps, int32_t* first, int32_t* ntaps,
                                  float* w, int32_t cap_phases, int64_t cap_w) {
    return guard([&] {
        NEED(iu); NEED(ou); NEED(max_taps);
        const ResamplePlan p = resample_plan(in_rate, out_rate);
        *iu = p.iu; *ou = p.ou; *max_taps = p.max_taps;
        if (!first && !ntaps && !w) return;   // (the sizes alone)
        if (p.ou > cap_phases || (w && (int64_t)p.w.size() > cap_w))
            failf(K2HIP_ERR_CAPACITY, "resample plan %d -> %d: %d phases x %d taps", in_rate, out_rate, p.ou, p.max_taps);
        if (first) memcpy(first, p.first.data(), sizeof(int32_t) * (size_t)p.ou);
        if (ntaps) memcpy(ntaps, p.ntaps.data(), sizeof(int32_t) * (size_t)p.ou);
        if (w) memcpy(w, p.w.data(), sizeof(float) * p.w.size());
    });
}
int64_t k2hip_debug_resample_num_out(int32_t in_rate, int32_t out_rate, int64_t n_in_total) {
    int64_t r = -1;
    guard([&] {
        K2_REQUIRE(n_in_total >= 0 && n_in_total < kResampleMaxInput, "resample_num_out: %lld samples", (long long)n_in_total);
        r = resample_plan(in_rate, out_rate).num_out(n_in_total);
    });
    return r;
}
int32_t k2hip_debug_resample_ref(int32_t in_rate, int32_t out_rate, float* tail, int64_t* n_tail, int64_t tail_cap, int64_t* n_in, int64_t* n_out,
                                 const float* x, int64_t n, float* out, int64_t cap, int64_t* n_written) {
    return guard([&] {
        NEED(n_tail); NEED(n_in); NEED(n_out); NEED(n_written);
        K2_REQUIRE(n >= 0 && *n_tail >= 0 && *n_tail <= *n_in && *n_out >= 0 && *n_in + n < kResampleMaxInput, "resample_ref: bad carried block");
        if (n > 0) NEED(x);
        if (*n_tail > 0) NEED(tail);
        const ResamplePlan p = resample_plan(in_rate, out_rate);
        K2_REQUIRE(*n_out == p.num_out(*n_in) && *n_in - *n_tail <= p.keep_from(*n_out), "resample_ref: the carried block does not belong to %lld "
                   "samples in, %lld out", (long long)*n_in, (long long)*n_out);
        ResampleRefState st;
        st.tail.assign(tail, tail + *n_tail);
        st.n_in = *n_in;
        st.n_out = *n_out;
        std::vector<float> y;
        resample_ref_push(p, st, x, n, &y);
        *n_written = (int64_t)y.size();
        if ((int64_t)y.size() > cap || (int64_t)st.tail.size() > tail_cap)
            failf(K2HIP_ERR_CAPACITY, "resample_ref: %zu outputs and a tail of %zu samples", y.size(), st.tail.size());
        if (!y.empty()) {
            NEED(out);
            memcpy(out, y.data(), sizeof(float) * y.size());
        }
        if (!st.tail.empty()) {
            NEED(tail);
            memcpy(tail, st.tail.data(), sizeof(float) * st.tail.size());
        }
        *n_tail = (int64_t)st.tail.size();
        *n_in = st.n_in;
        *n_out = st.n_out;
    });
}
// the plans a model has built so far (one per input rate that differed from its own)
int32_t k2hip_debug_resample_plans(k2hip_model_t* model, int32_t* n) {
    return guard([&] {
        NEED(model); NEED(n);
        std::lock_guard<std::mutex> lk(model->rs_mu);
        *n = (int32_t)model->rs_plans.size();
    });
}
// B AddSamples calls over the rows of one [B, n] matrix (row stride in floats): what a host that receives audio in lock step
// holds anyway; saves building B pointers per 50 ms push
int32_t k2hip_online_accept_samples_matrix(k2hip_model_t* model, k2hip_online_stream_t* const* streams, int32_t B, const float* samples,
                                           int64_t row_stride, int64_t n) {
    return guard([&] {
        NEED(model); NEED(streams);
        K2_REQUIRE(B > 0 && n >= 0 && row_stride >= n, "accept_samples_matrix: bad shape");
        if (n > 0) NEED(samples);
        for (int i = 0; i < B; i++) {
            NEED(streams[i]);
            online_add_samples(streams[i], samples + (size_t)i * row_stride, n);
        }
    });
}
int32_t k2hip_online_stream_accept_features(k2hip_online_stream_t* s, const float* feats, int64_t n_frames) {
    return guard([&] {
        NEED(s);
        if (n_frames > 0) NEED(feats);
        const int feat = s->model->engine.model().cfg().feat;
        online_materialize(&s, 1);  // frames of samples accepted earlier come first
        if (n_frames > 0) {
            const int64_t have = (int64_t)(s->speech.size() / (size_t)feat);
            if (s->mir_ok && have + n_frames > Engine::kFifoFrames) s->mir_ok = false;
            if (s->mir_ok) {
                Engine& e = s->model->engine;
                EngineLock lk(e);
                e.online_fifo_write(s->slot, (int)((s->mir_head + have) % Engine::kFifoFrames), feats, n_frames);
            }
        }
        s->speech.insert(s->speech.end(), feats, feats + n_frames * feat);
    });
}
int64_t k2hip_online_stream_speech_length(const k2hip_online_stream_t* s) { return s ? online_logical_floats(s) : -1; }
// the feature FIFO itself: the frames of samples accepted earlier are materialised first
int32_t k2hip_online_stream_get_speech(k2hip_online_stream_t* s, float* out, int64_t cap) {
    return guard([&] {
        NEED(s);
        online_materialize(&s, 1);
        if ((int64_t)s->speech.size() > cap) failf(K2HIP_ERR_CAPACITY, "speech has %zu floats", s->speech.size());
        if (!s->speech.empty()) {
            NEED(out);
            memcpy(out, s->speech.data(), sizeof(float) * s->speech.size());
        }
    });
}
// OnlineStream.IsFinished (:124-161)
int32_t k2hip_online_stream_is_finished(k2hip_online_stream_t* s, int32_t is_endpoint, int32_t* finished) {
    return guard([&] {
        NEED(s); NEED(finished);
        const Config& c = s->model->engine.model().cfg();
        *finished = 0;
        if (!is_endpoint) return;
        online_materialize(&s, 1);  // the test below looks at the feature VALUES
        const size_t oLen = s->speech.size();
        if (oLen == 0) { *finished = 1; return; }
        double sum = 0.0;   // LINQ Average() over float[] accumulates in double and returns float
        for (float v : s->speech) sum += v;
        const float avg = (float)(sum / (double)oLen);
        size_t num = 0;
        for (float v : s->speech) num += (v != avg);
        if (num == 0) { *finished = 1; return; }
        if ((long long)oLen <= (long long)c.chunk_T * c.feat) {
            // AddSamples(new float[400]) (:146); a resampling stream takes them at its own rate, ceil(400 iu / ou) zeros
            const int64_t nz = s->rs ? (400 * (int64_t)s->rs->iu + s->rs->ou - 1) / s->rs->ou : 400;
            std::vector<float> z((size_t)nz, 0.f);
            if (s->rs) online_add_waveform(s, s->rate, z.data(), nz);
            else online_add_samples(s, z.data(), nz);
        }
    });
}
// OnlineRecognizer.ForwardBatchGreedySearch (:85-219)
int32_t k2hip_online_step(k2hip_model_t* model, k2hip_online_stream_t* const* streams, int32_t B, int32_t* decoded, int32_t* n_new_tokens) {
    return guard([&] {
        NEED(model); NEED(streams); NEED(decoded); NEED(n_new_tokens);
        Engine& e = model->engine;
        const Config& c = e.model().cfg();
        K2_REQUIRE(c.streaming || c.lstm, "this model is not a streaming export");
        if (c.ctc) {   // (before any stream is looked at: nothing changes)
            EngineLock lk(e);
            K2_REQUIRE(e.ctc_prefix() == 0, "online step: the decoding method is ctc_prefix_beam_search (beam %d), which covers the offline "
                       "entries only -- set greedy_search for streaming", e.ctc_prefix());
        }
        const size_t chunk_floats = (size_t)c.chunk_T * c.feat, shift_floats = (size_t)c.shift * c.feat;
        uint64_t lm_serial = 0;   // the n-gram LM this tick's beam search runs with (0 = none) and its start state
        int lm_start = 0;
        int K = 0;   // the search of this tick: 0 = greedy (and a CTC model's own search), K = modified beam search with beam K
        NlmStreamCall nlm;   // the neural LM fusion setting this tick's beam search runs with
        uint64_t lodr_serial = 0;   // the LODR setting this tick's beam search runs with (0 = none, or no active fusion), its start state
        int lodr_start = 0;
        if (!c.ctc) {
            EngineLock lk(e);
            K = e.beam();
            K2_REQUIRE(K > 0 || e.nbest() == 0, "online step: the model keeps %d alternatives (k2hip_set_nbest) but decodes with greedy_search, "
                       "which has none", e.nbest());
            K2_REQUIRE(!(K > 0 && e.has_hotwords()),
                       "online step: hotword biasing covers the offline modified beam search only, not the streaming one -- clear the "
                       "hotwords (k2hip_set_hotwords(model, NULL)) or decode with greedy_search");
            lm_serial = K > 0 ? model->lm_serial : 0;
            lm_start = model->lm_start;
            if (K > 0) nlm.read(model);
            lodr_serial = nlm.active ? model->lodr_serial : 0;   // (LODR acts only beside the neural LM)
            lodr_start = lodr_serial ? model->lodr_host->start : 0;
        }
        std::vector<int> idx;
        int CK = 0;   // a CTC model's streams under the carried prefix search: their beam (every stream of the list carries the same setting)
        for (int i = 0; i < B; i++) {
            NEED(streams[i]);
            K2_REQUIRE(streams[i]->model == model, "stream %d belongs to another model", i);
            K2_REQUIRE(streams[i]->cp_beam == streams[0]->cp_beam, "online step: stream %d has ctc_prefix_beam %d, stream 0 has %d -- every stream "
                       "of one call carries the same setting (k2hip_online_stream_set_ctc_prefix_beam)", i, streams[i]->cp_beam, streams[0]->cp_beam);
            K2_REQUIRE(!streams[i]->poisoned, "stream %d took part in a chunk step that failed: its caches are undefined, reset it first", i);
            K2_REQUIRE(streams[i]->method < 0 || streams[i]->method == K,
                       "stream %d started decoding with %s (beam %d); the decoding method changed since -- reset the stream first", i,
                       streams[i]->method > 0 ? "modified_beam_search" : "greedy_search", streams[i]->method);
            decoded[i] = 0;
            n_new_tokens[i] = 0;
            if ((size_t)online_logical_floats(streams[i]) >= chunk_floats) idx.push_back(i);   // GetDecodeChunk (:82-100)
        }
        {   // one stream twice in the list would consume two chunks against one state slot in the same launch
            std::vector<const k2hip_online_stream*> seen(streams, streams + B);
            std::sort(seen.begin(), seen.end());
            K2_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "GetResults: the same stream appears twice in the list");
        }
        if (idx.empty()) return;   // :113-116
        CK = streams[0]->cp_beam;
        // the carried prefix search with biasing: per stream, opt-in; the LM rule of the beam search holds for the streams that opted in
        bool cp_bias = false;
        CtcPrefixBiasCall cpb;
        for (size_t r = 0; CK > 0 && r < idx.size(); r++) cp_bias = cp_bias || streams[idx[r]]->cp_biasing;
        if (cp_bias) {
            {
                EngineLock lk(e);
                cpb.lm_serial = model->lm_serial; cpb.lm_start = model->lm_start; cpb.lm_states = model->lm_states;
            }
            for (size_t r = 0; r < idx.size(); r++) {
                const k2hip_online_stream* s = streams[idx[r]];
                if (s->cp_biasing && s->cprefix) CtcPrefixBiasCall::check_lm(*s->cprefix, cpb.lm_serial, "online step", idx[r]);
            }
        }
        // a stream keeps the LM it decoded its first chunk with (decided for all streams before anything of any of them moves)
        for (size_t r = 0; K > 0 && r < idx.size(); r++) {
            const k2hip_online_stream* s = streams[idx[r]];
            K2_REQUIRE(!s->beam || s->beam->frames() == 0 || s->beam->lm_serial() == lm_serial,
                       "online step: stream %d has decoded %lld frames with another n-gram LM setting (k2hip_set_ngram_lm changed or cleared "
                       "it) and its hypotheses carry that LM's states -- reset the stream first", idx[r], s->beam->frames());
            nlm.check(s->nlm.get(), s->beam ? s->beam->frames() : 0, "online step", idx[r]);
            K2_REQUIRE(!s->beam || s->beam->frames() == 0 || s->beam->lodr_serial() == lodr_serial,
                       "online step: stream %d has decoded %lld frames with another LODR setting (k2hip_set_lodr_lm changed or cleared it) and "
                       "its hypotheses carry that LM's states -- reset the stream first", idx[r], s->beam->frames());
        }
        // the new frames' host copy is collected after the step (one wait for the device per tick); whatever way this call ends -- an
        // allocation failure below included -- the outstanding download is collected before the streams' Speech can move
        // If the collection itself fails (the device work behind the download did), the streams whose Speech was extended with
        // placeholder frames for it are poisoned: their FIFOs hold zeros where audio should be, and a later step must not decode them.
        struct GatherFinisher {
            Engine& e;
            std::vector<k2hip_online_stream*> owners;   // the streams whose frames the outstanding download carries
            bool armed = false;
            void finish() {
                if (!armed) return;
                armed = false;
                try {
                    EngineLock lk(e);
                    e.fbank_gather_finish();
                } catch (...) {
                    for (k2hip_online_stream* s : owners) s->poisoned = true;
                    throw;
                }
            }
            ~GatherFinisher() {
                try { finish(); } catch (...) {}   // (already unwinding, or the caller is done: the streams are poisoned, the error of record is the first one)
            }
        } fb{e};
        {   // the deferred fbank of the streams that decode now: one batched launch when they are at the same position
            std::vector<k2hip_online_stream*> ready(idx.size());
            for (size_t r = 0; r < idx.size(); r++) ready[r] = streams[idx[r]];
            fb.owners = ready;
            fb.armed = online_materialize(ready.data(), (int)ready.size(), true);
        }
        const int R = (int)idx.size(), Tp = e.online_frames_per_chunk();
        std::vector<const float*> chunks(R);   // GetDecodeChunk: the first ChunkLength frames of each FIFO
        std::vector<int> slots(R);
        std::vector<long long> hyps(2 * (size_t)R), plens(R);
        std::vector<int> nch(R), heads(R);
        bool all_mirrored = true;
        for (int r = 0; r < R; r++) {
            k2hip_online_stream* s = streams[idx[r]];
            heads[r] = s->mir_head;
            all_mirrored = all_mirrored && s->mir_ok;
            chunks[r] = s->speech.data();
            slots[r] = s->slot;
            hyps[2 * r] = s->hyp[0];
            hyps[2 * r + 1] = s->hyp[1];
            plens[r] = s->processed_len;
            nch[r] = (int)(s->chunks_done % (1LL << 30));  // the kernels only need it modulo the ring lengths; (1 << 30) % KL drift is
                                                           // irrelevant before 2^30 chunks (~10 years of audio)
        }
        std::vector<int64_t> tok;
        std::vector<int32_t> ts, n;
        std::vector<int> bin, bout;   // modified beam search: the streams' saved hypotheses in, the surviving ones out
        bool any_hw = false;
        const bool with_lm = lm_serial != 0, with_lodr = lodr_serial != 0;
        const int planes = 1 + (with_lm ? 1 : 0) + (with_lodr ? 1 : 0);   // graph states | LM states | LODR states
        std::vector<BeamHwStream> graphs;
        std::vector<int> st_in, st_out;
        const BeamResumeLayout RL{std::max(K, 1), Tp};
        if (K > 0) {
            bin.resize((size_t)R * RL.in_ints());
            bout.resize((size_t)R * RL.out_ints());
            for (int r = 0; r < R; r++) {
                k2hip_online_stream* s = streams[idx[r]];
                if (!s->beam) {
                    s->beam.reset(new BeamHistory(K, K2HIP_BLANK_ID));
                    if (s->hw) s->beam->set_pending(s->hw->pending);
                }
                if (s->beam->frames() == 0) {
                    s->beam->begin_lm(lm_serial, with_lm ? lm_start : 0);
                    s->beam->begin_lodr(lodr_serial, lodr_start);
                    nlm.begin(s->nlm);
                }
                s->beam->fill_in(bin.data() + (size_t)r * RL.in_ints(), Tp);
                any_hw = any_hw || s->hw;
            }
            any_hw = any_hw || with_lm || with_lodr;   // (the LM and LODR states ride in the same side blocks, behind the graph states)
            if (any_hw) {   // hotword graphs / LM: the side blocks of the tick (neither anywhere: the unbiased call, unchanged)
                graphs.resize((size_t)R);
                st_in.resize((size_t)R * K * planes);
                st_out.resize((size_t)R * K * planes);
                for (int r = 0; r < R; r++) {
                    k2hip_online_stream* s = streams[idx[r]];
                    if (s->hw) graphs[(size_t)r] = s->hw->tables;
                    s->beam->fill_states(st_in.data() + (size_t)r * K);
                    if (with_lm) s->beam->fill_lm_states(st_in.data() + (size_t)(R + r) * K);
                    if (with_lodr) s->beam->fill_lodr_states(st_in.data() + ((size_t)(planes - 1) * R + r) * K);
                }
            }
        } else if (CK > 0) {   // the carried prefixes in, the survivors out
            const CtcPrefixResumeLayout CL{CK, Tp};
            bin.resize((size_t)R * CL.in_ints());
            bout.resize((size_t)R * CL.out_ints());
            for (int r = 0; r < R; r++) {
                k2hip_online_stream* s = streams[idx[r]];
                if (!s->cprefix) s->cprefix.reset(new CtcPrefixHistory(CK, s->cp_nbest));   // (the start state: as good as none)
                s->cprefix->fill_in(bin.data() + (size_t)r * CL.in_ints(), Tp);
            }
            if (cp_bias) {   // some stream of the tick is biased: graphs and side blocks for the whole call
                cpb.stage(R, CK);
                for (int r = 0; r < R; r++) {
                    k2hip_online_stream* s = streams[idx[r]];
                    cpb.fill(r, CK, *s->cprefix, s->hw.get(), s->cp_biasing);
                }
            }
        } else {
            tok.resize((size_t)R * Tp);
            ts.resize((size_t)R * Tp);
            n.resize(R);
        }
        if (!all_mirrored) fb.finish();   // the step reads some stream's chunk from host memory: the frames must be there
        std::vector<float> ypb;   // N-best on: the token log-probs of the survivors' suffixes come back beside the out blocks
        bool lm_raced = false;
        try {
            EngineLock lk(e);
            // the LM states staged above index the tables of setting lm_serial: this lock covers the launch, and k2hip_set_ngram_lm
            // takes it too, so a setting that changed since it was read is caught here, before any device work
            if ((K > 0 && model->lm_serial != lm_serial) || (cp_bias && model->lm_serial != cpb.lm_serial)) {
                lm_raced = true;
                failf(K2HIP_ERR_INVALID, "online step: k2hip_set_ngram_lm changed the n-gram LM while this step was being prepared; call again");
            }
            struct YpOut {
                Engine& e;
                ~YpOut() { e.set_beam_yp_out(nullptr); }
            } yp_guard{e};
            if (K > 0 && e.nbest() > 0) {
                ypb.resize((size_t)R * K * Tp);
                e.set_beam_yp_out(ypb.data());
            }
            struct NlmOut {
                Engine& e;
                ~NlmOut() { e.set_beam_nlm_io(nullptr); }
            } nlm_guard{e};
            if (K > 0 && (model->rnn_serial != nlm.serial || e.rnn_lm_stream_fusion_active() != nlm.active)) {
                lm_raced = true;
                failf(K2HIP_ERR_INVALID, "online step: the neural LM fusion setting changed while this step was being prepared; call again");
            }
            if (K > 0 && (nlm.active ? model->lodr_serial : 0) != lodr_serial) {   // (k2hip_set_lodr_lm takes this lock too)
                lm_raced = true;
                failf(K2HIP_ERR_INVALID, "online step: k2hip_set_lodr_lm changed the LODR LM while this step was being prepared; call again");
            }
            if (nlm.active) {   // the streams' state blocks (taken at a stream's first fused chunk), staged with the in blocks
                try {
                    for (int r = 0; r < R; r++) nlm.stage(model, r, R, K, *streams[idx[r]]->nlm);
                } catch (...) {
                    lm_raced = true;   // (no device work has been enqueued: the streams are as they were)
                    throw;
                }
                e.set_beam_nlm_io(nlm.table.data());
            }
            if (K > 0 && any_hw)
                e.online_step_beam_hw(slots.data(), chunks.data(), plens.data(), nch.data(), R, K, bin.data(), bout.data(),
                                      Engine::BeamHwIO{graphs.data(), st_in.data(), st_out.data(), with_lm, with_lodr}, all_mirrored ? heads.data() : nullptr);
            else if (K > 0)
                e.online_step_beam(slots.data(), chunks.data(), plens.data(), nch.data(), R, K, bin.data(), bout.data(),
                                   all_mirrored ? heads.data() : nullptr);
            else if (CK > 0) {
                if (cp_bias)
                    e.online_step_ctc_prefix_bias(slots.data(), chunks.data(), plens.data(), nch.data(), R, CK, bin.data(), bout.data(),
                                                  Engine::CtcPrefixBiasIO{cpb.graphs.data(), cpb.side_in.data(), cpb.side_out.data(), cpb.with_lm()},
                                                  all_mirrored ? heads.data() : nullptr);
                else
                    e.online_step_ctc_prefix(slots.data(), chunks.data(), plens.data(), nch.data(), R, CK, bin.data(), bout.data(),
                                             all_mirrored ? heads.data() : nullptr);
                const CtcPrefixResumeLayout CL{CK, Tp};   // (the device work is done: an out block that fails its check poisons the streams)
                const CtcPrefixResumeBiasLayout SL{CK};
                for (int r = 0; r < R; r++) {
                    const k2hip_online_stream* s = streams[idx[r]];
                    if (cp_bias && s->cp_biasing)
                        s->cprefix->check_out(bout.data() + (size_t)r * CL.out_ints(), cpb.side_out.data() + (size_t)r * SL.out_ints(), Tp, Tp,
                                              CtcPrefixBiasCall::graph_states(s->hw.get(), true), cpb.with_lm() ? cpb.lm_states : 0);
                    else s->cprefix->check_out(bout.data() + (size_t)r * CL.out_ints(), Tp, Tp);
                }
            } else
                e.online_step(slots.data(), chunks.data(), hyps.data(), plens.data(), nch.data(), R, tok.data(), ts.data(), n.data(),
                              all_mirrored ? heads.data() : nullptr);
        } catch (...) {
            // Host-side nothing has moved (RemoveChunk happens below), but the device caches of these streams may have: the step
            // updates the conv / embed caches in place.  A search exchange timeout is retried inside the engine and does not come
            // here; what does is a HIP failure.  The streams are unusable until reset.
            for (int r = 0; r < R && !lm_raced; r++) streams[idx[r]]->poisoned = true;   // (the LM race is decided before any device work)
            throw;   // (fb's destructor collects the frames; the streams are poisoned either way)
        }
        fb.finish();   // the step's token download has synchronised the stream: copies only
        nlm.done = true;
        // RemoveChunk (:102-117) only after success
        std::vector<k2hip_online_stream*> remirror;
        for (int r = 0; r < R; r++) {
            k2hip_online_stream* s = streams[idx[r]];
            s->speech.erase(s->speech.begin(), s->speech.begin() + shift_floats);
            s->mir_head = (s->mir_head + c.shift) % Engine::kFifoFrames;
            if (!s->mir_ok && s->speech.size() / (size_t)c.feat <= (size_t)Engine::kFifoFrames) {
                // the FIFO fits its device ring again (a host that pushed a whole file before decoding, as the reference's example
                // does, never drains it to empty: a step needs ChunkLength frames and removes only ShiftLength): re-upload what is
                // left at ring row 0 and the stream is back on the one-upload-per-tick path
                remirror.push_back(s);
            }
            s->chunks_done++;
            s->method = K;
            if (K > 0) {
                // the best hypothesis replaces the result (it may revise earlier tokens): n_new_tokens = change of its length
                const int64_t before = (int64_t)s->beam->tokens().size();
                const float* yp = ypb.empty() ? nullptr : ypb.data() + (size_t)r * K * Tp;
                if (nlm.active) nlm.flip(*s->nlm);
                if (any_hw) s->beam->apply_out_states(bout.data() + (size_t)r * RL.out_ints(), Tp, st_out.data() + (size_t)r * K, yp,
                                                      with_lm ? st_out.data() + (size_t)(R + r) * K : nullptr,
                                                      with_lodr ? st_out.data() + ((size_t)(planes - 1) * R + r) * K : nullptr);
                else s->beam->apply_out(bout.data() + (size_t)r * RL.out_ints(), Tp, yp);
                s->hyp[0] = s->beam->hyp_last(0);
                s->hyp[1] = s->beam->hyp_last(1);
                n_new_tokens[idx[r]] = (int32_t)((int64_t)s->beam->tokens().size() - before);
            }
            if (CK > 0) {   // the best prefix replaces the result (it may revise earlier tokens): n_new_tokens = change of its length
                const CtcPrefixResumeLayout CL{CK, Tp};
                const int64_t before = (int64_t)s->cprefix->tokens().size();
                // (a biased stream reports the first entry in final order: its tokens are revised more often than the unbiased search's)
                if (cp_bias && s->cp_biasing)
                    s->cprefix->apply_out(bout.data() + (size_t)r * CL.out_ints(), cpb.side_out.data() + (size_t)r * CtcPrefixResumeBiasLayout{CK}.out_ints(), Tp, Tp);
                else s->cprefix->apply_out(bout.data() + (size_t)r * CL.out_ints(), Tp, Tp);
                s->tokens.assign(2, K2HIP_BLANK_ID);
                s->tokens.insert(s->tokens.end(), s->cprefix->tokens().begin(), s->cprefix->tokens().end());
                s->timestamps = s->cprefix->timestamps();
                n_new_tokens[idx[r]] = (int32_t)((int64_t)s->cprefix->tokens().size() - before);
            }
            for (int k = 0; K == 0 && CK == 0 && k < n[r]; k++) {
                s->tokens.push_back(tok[(size_t)r * Tp + k]);          // :183
                s->timestamps.push_back(ts[(size_t)r * Tp + k]);       // :184 (chunk-relative frame index)
            }
            if (!c.ctc && K == 0) {  // the CTC delegate leaves Hyp alone (OnlineRecognizer.cs:302-310)
                s->hyp[0] = s->tokens[s->tokens.size() - 2];           // :208
                s->hyp[1] = s->tokens[s->tokens.size() - 1];
            }
            if (c.conformer) s->processed_len = R;   // OnlineProjOfConformer.unstack_states (:229) stores the BATCH SIZE (sic), not the model's output
            else if (c.zip1) s->processed_len += (c.chunk_T - 7) / 2;  // no processed_lens state in v1; kept as a frame counter
            else s->processed_len += (c.chunk_T - 7) / 2 - 3;      // new_processed_lens = processed_lens + x_lens
            decoded[idx[r]] = 1;
            if (K == 0 && CK == 0) n_new_tokens[idx[r]] = n[r];
        }
        if (!remirror.empty()) {
            EngineLock lk(e);
            for (k2hip_online_stream* s : remirror) {
                const int64_t have = (int64_t)(s->speech.size() / (size_t)c.feat);
                if (have > 0) e.online_fifo_write(s->slot, 0, s->speech.data(), have);
                s->mir_head = 0;
                s->mir_ok = true;
            }
        }
    });
}
// ---- operator level of the streaming path (IOnlineProj.cs:65-71) --------------------------------------------------------------
// GetEncoderInitStates for ONE stream (OnlineProjOfZipformer2.cs:144-238): a zeroed slot
int32_t k2hip_online_state_create(k2hip_model_t* model, k2hip_online_state_t** out) {
    return guard([&] {
        NEED(model); NEED(out);
        const Config& c = model->engine.model().cfg();
        K2_REQUIRE(c.streaming && !c.lstm && !c.conformer && !c.zip1, "online states: streaming Zipformer2 models only");
        auto* st = new k2hip_online_state();
        st->model = model;
        try {
            EngineLock lk(model->engine);
            st->slot = model->engine.online_alloc_slot();
        } catch (...) {
            delete st;
            throw;
        }
        *out = st;
    });
}
int32_t k2hip_online_state_destroy(k2hip_online_state_t* st) {
    return guard([&] {
        if (!st) return;
        {
            EngineLock lk(st->model->engine);
            st->model->engine.online_free_slot(st->slot);
        }
        delete st;
    });
}
int64_t k2hip_online_state_processed_len(const k2hip_online_state_t* st) { return st ? (int64_t)st->processed_len : -1; }
// EncoderProj (OnlineProjOfZipformer2.cs:491-618) over B states: feats [B, ChunkLength, FeatureDim] (raw fbank: the log floor of the
// online PadSequence is applied inside), encoder_out [B, T', joiner_dim]; the states advance in place, so stack_states /
// unstack_states (:240-489) are the identity on the handles
int32_t k2hip_online_encoder(k2hip_model_t* model, k2hip_online_state_t* const* states, int32_t B, const float* feats, float* encoder_out,
                             int64_t cap_floats) {
    return guard([&] {
        NEED(model); NEED(states); NEED(feats); NEED(encoder_out);
        K2_REQUIRE(B > 0, "EncoderProj: empty batch");
        Engine& e = model->engine;
        const Config& c = e.model().cfg();
        const int Tp = e.online_frames_per_chunk();
        if (cap_floats < (int64_t)B * Tp * c.enc_dim()) failf(K2HIP_ERR_CAPACITY, "encoder_out needs %lld floats", (long long)B * Tp * c.enc_dim());
        std::vector<int> slots(B), nch(B);
        std::vector<long long> plens(B);
        {
            std::vector<const k2hip_online_state*> seen(states, states + B);
            for (int b = 0; b < B; b++) {
                NEED(states[b]);
                K2_REQUIRE(states[b]->model == model, "state %d belongs to another model", b);
                K2_REQUIRE(!states[b]->poisoned, "state %d took part in an EncoderProj call that failed: its caches are undefined, re-create it", b);
            }
            std::sort(seen.begin(), seen.end());
            K2_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "EncoderProj: the same state appears twice in the batch");
        }
        for (int b = 0; b < B; b++) {
            slots[b] = states[b]->slot;
            plens[b] = states[b]->processed_len;
            nch[b] = (int)(states[b]->chunks_done % (1LL << 30));
        }
        try {
            EngineLock lk(e);
            e.online_encoder(slots.data(), feats, plens.data(), nch.data(), B, encoder_out);
        } catch (...) {
            for (int b = 0; b < B; b++) states[b]->poisoned = true;  // the conv / embed caches may have advanced in place
            throw;
        }
        for (int b = 0; b < B; b++) {  // only after success, as in k2hip_online_step
            states[b]->chunks_done++;
            states[b]->processed_len += (c.chunk_T - 7) / 2 - 3;
        }
    });
}

int64_t k2hip_online_stream_processed_len(const k2hip_online_stream_t* s) { return s ? (int64_t)s->processed_len : -1; }
// Tokens / Timestamps: the greedy stream's own lists, or the best hypothesis of a stream under modified_beam_search
static const std::vector<int64_t>& online_tokens(const k2hip_online_stream* s) { return s->method > 0 ? s->beam->tokens() : s->tokens; }
static const std::vector<int32_t>& online_timestamps(const k2hip_online_stream* s) { return s->method > 0 ? s->beam->timestamps() : s->timestamps; }
int32_t k2hip_online_stream_num_tokens(const k2hip_online_stream_t* s) { return s ? (int32_t)online_tokens(s).size() : -1; }
int32_t k2hip_online_stream_num_timestamps(const k2hip_online_stream_t* s) { return s ? (int32_t)online_timestamps(s).size() : -1; }
int32_t k2hip_online_stream_get_tokens(const k2hip_online_stream_t* s, int64_t* tokens, int32_t cap) {
    return guard([&] {
        NEED(s);
        const std::vector<int64_t>& t = online_tokens(s);
        if ((int)t.size() > cap) failf(K2HIP_ERR_CAPACITY, "stream holds %zu tokens", t.size());
        if (!t.empty()) { NEED(tokens); memcpy(tokens, t.data(), sizeof(int64_t) * t.size()); }
    });
}
int32_t k2hip_online_stream_get_timestamps(const k2hip_online_stream_t* s, int32_t* timestamps, int32_t cap) {
    return guard([&] {
        NEED(s);
        const std::vector<int32_t>& t = online_timestamps(s);
        if ((int)t.size() > cap) failf(K2HIP_ERR_CAPACITY, "stream holds %zu timestamps", t.size());
        if (!t.empty()) { NEED(timestamps); memcpy(timestamps, t.data(), sizeof(int32_t) * t.size()); }
    });
}
int32_t k2hip_online_stream_get_score(const k2hip_online_stream_t* s, float* score) {
    return guard([&] {
        NEED(s); NEED(score);
        if (s->cp_beam > 0) {   // a CTC stream under the carried prefix search: the best prefix' total (0 before its first chunk)
            *score = s->cprefix ? s->cprefix->score() : 0.f;
            return;
        }
        K2_REQUIRE(s->method != 0, "the stream decodes with greedy_search: it has no hypothesis score");
        *score = s->method > 0 ? s->beam->score() : 0.f;   // (no chunk yet: the start hypothesis, log-prob 0)
    });
}

// ---- operator level of the streaming beam search ---------------------------------------------------------------------------------
int32_t k2hip_beam_stream_create(k2hip_model_t* model, int32_t beam, k2hip_beam_stream_t** out) {
    return guard([&] {
        NEED(model); NEED(out);
        *out = nullptr;
        K2_REQUIRE(beam >= 1 && beam <= kMaxBeam, "beam stream: beam %d out of range [1,%d]", beam, kMaxBeam);
        K2_REQUIRE(!model->engine.model().cfg().ctc, "beam stream: a CTC model has no transducer search");
        *out = new k2hip_beam_stream{model, BeamHistory(beam, K2HIP_BLANK_ID), nullptr};
    });
}
int32_t k2hip_beam_stream_destroy(k2hip_beam_stream_t* s) {
    return guard([&] { delete s; });
}
int32_t k2hip_beam_stream_reset(k2hip_beam_stream_t* s) {
    return guard([&] {
        NEED(s);
        s->hist.reset();   // (an attached hotword graph stays; every hypothesis is back at its root)
        s->nlm.reset();    // (the LM state block goes back to the model's pool, or is forgotten when the model is gone)
    });
}
int32_t k2hip_beam_stream_set_hotwords(k2hip_beam_stream_t* s, const k2hip_hotwords_t* hw) {
    return guard([&] {
        NEED(s);
        K2_REQUIRE(s->hist.frames() == 0, "beam stream set_hotwords: the stream has searched %lld frames and its hypotheses carry states of the "
                   "graph it started with -- reset the stream first", s->hist.frames());
        s->hw = hw ? hw_resident_get(s->model, hw, "beam stream set_hotwords") : nullptr;
        s->hist.set_pending(s->hw ? s->hw->pending : nullptr);
    });
}
int32_t k2hip_beam_search_chunk(k2hip_model_t* model, k2hip_beam_stream_t* const* streams, int32_t B, const float* enc_out, int32_t Tc) {
    return guard([&] {
        NEED(model); NEED(streams); NEED(enc_out);
        K2_REQUIRE(B > 0 && Tc >= 1, "beam search chunk: bad shape B=%d Tc=%d", B, Tc);
        uint64_t lm_serial = 0;   // the n-gram LM this call runs with (0 = none) and its start state
        int lm_start = 0;
        NlmStreamCall nlm;        // the neural LM fusion setting this call runs with
        uint64_t lodr_serial = 0; // the LODR setting this call runs with (0 = none, or no active fusion) and its start state
        int lodr_start = 0;
        {
            EngineLock lk(model->engine);
            K2_REQUIRE(!model->engine.has_hotwords(), "beam search chunk: hotword biasing covers the offline modified beam search only, not the "
                                                      "streaming one -- clear the hotwords (k2hip_set_hotwords(model, NULL)) first");
            lm_serial = model->lm_serial;
            lm_start = model->lm_start;
            nlm.read(model);
            // (LODR acts only beside the neural LM: without an active streaming fusion the setting is ignored, as if none were set)
            lodr_serial = nlm.active ? model->lodr_serial : 0;
            lodr_start = lodr_serial ? model->lodr_host->start : 0;
        }
        std::vector<const k2hip_beam_stream*> seen(streams, streams + B);
        for (int b = 0; b < B; b++) {
            NEED(streams[b]);
            K2_REQUIRE(streams[b]->model == model, "beam stream %d belongs to another model", b);
            K2_REQUIRE(streams[b]->hist.beam() == streams[0]->hist.beam(), "beam stream %d has beam %d, stream 0 has %d: one beam per call", b,
                       streams[b]->hist.beam(), streams[0]->hist.beam());
        }
        std::sort(seen.begin(), seen.end());
        K2_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "beam search chunk: the same stream appears twice");
        const int K = streams[0]->hist.beam();
        const bool with_lm = lm_serial != 0;
        // a stream keeps the LM it searched its first chunk with (decided for all streams before any of them changes)
        for (int b = 0; b < B; b++)
            K2_REQUIRE(streams[b]->hist.frames() == 0 || streams[b]->hist.lm_serial() == lm_serial,
                       "beam search chunk: stream %d has searched %lld frames with another n-gram LM setting (k2hip_set_ngram_lm changed or "
                       "cleared it) and its hypotheses carry that LM's states -- reset the stream first", b, streams[b]->hist.frames());
        for (int b = 0; b < B; b++) nlm.check(streams[b]->nlm.get(), streams[b]->hist.frames(), "beam search chunk", b);
        const bool with_lodr = lodr_serial != 0;
        for (int b = 0; b < B; b++)
            K2_REQUIRE(streams[b]->hist.frames() == 0 || streams[b]->hist.lodr_serial() == lodr_serial,
                       "beam search chunk: stream %d has searched %lld frames with another LODR setting (k2hip_set_lodr_lm changed or cleared "
                       "it) and its hypotheses carry that LM's states -- reset the stream first", b, streams[b]->hist.frames());
        for (int b = 0; b < B; b++)
            if (streams[b]->hist.frames() == 0) {
                streams[b]->hist.begin_lm(lm_serial, with_lm ? lm_start : 0);
                streams[b]->hist.begin_lodr(lodr_serial, lodr_start);
                nlm.begin(streams[b]->nlm);
            }
        const BeamResumeLayout L{K, Tc};
        std::vector<int> bin((size_t)B * L.in_ints()), bout((size_t)B * L.out_ints());
        for (int b = 0; b < B; b++) streams[b]->hist.fill_in(bin.data() + (size_t)b * L.in_ints(), Tc);
        // hotword graphs / LM: with neither anywhere this is the unbiased call, unchanged; else the side blocks go along (the LM states
        // behind the graph states)
        bool any_hw = with_lm || with_lodr;
        for (int b = 0; b < B; b++) any_hw = any_hw || streams[b]->hw;
        std::vector<BeamHwStream> graphs;
        std::vector<int> st_in, st_out;
        const int planes = 1 + (with_lm ? 1 : 0) + (with_lodr ? 1 : 0);   // graph states | LM states | LODR states
        if (any_hw) {
            graphs.resize((size_t)B);
            st_in.resize((size_t)B * K * planes);
            st_out.resize((size_t)B * K * planes);
            for (int b = 0; b < B; b++) {
                if (streams[b]->hw) graphs[(size_t)b] = streams[b]->hw->tables;
                streams[b]->hist.fill_states(st_in.data() + (size_t)b * K);
                if (with_lm) streams[b]->hist.fill_lm_states(st_in.data() + (size_t)(B + b) * K);
                if (with_lodr) streams[b]->hist.fill_lodr_states(st_in.data() + ((size_t)(planes - 1) * B + b) * K);
            }
        }
        std::vector<float> ypb;
        {
            EngineLock lk(model->engine);
            struct YpOut {
                Engine& e;
                ~YpOut() { e.set_beam_yp_out(nullptr); }
            } yp_guard{model->engine};
            // (this lock covers the launch and k2hip_set_ngram_lm takes it too: the staged LM states still index the tables that are set)
            K2_REQUIRE(model->lm_serial == lm_serial, "beam search chunk: k2hip_set_ngram_lm changed the n-gram LM while this call was being "
                                                      "prepared; call again");
            if (model->engine.nbest() > 0) {
                ypb.resize((size_t)B * K * Tc);
                model->engine.set_beam_yp_out(ypb.data());
            }
            struct NlmOut {
                Engine& e;
                ~NlmOut() { e.set_beam_nlm_io(nullptr); }
            } nlm_guard{model->engine};
            K2_REQUIRE(model->rnn_serial == nlm.serial && model->engine.rnn_lm_stream_fusion_active() == nlm.active,
                       "beam search chunk: the neural LM fusion setting changed while this call was being prepared; call again");
            // (... and k2hip_set_lodr_lm takes this lock too: the staged LODR states still index the tables that are set)
            K2_REQUIRE((nlm.active ? model->lodr_serial : 0) == lodr_serial, "beam search chunk: k2hip_set_lodr_lm changed the LODR LM while "
                                                                             "this call was being prepared; call again");
            if (nlm.active) {   // the streams' state blocks (taken at a stream's first fused chunk), staged with the in blocks
                for (int b = 0; b < B; b++) nlm.stage(model, b, B, K, *streams[b]->nlm);
                model->engine.set_beam_nlm_io(nlm.table.data());
            }
            if (any_hw) model->engine.beam_chunk_host_hw(enc_out, B, Tc, K, bin.data(), bout.data(), Engine::BeamHwIO{graphs.data(), st_in.data(), st_out.data(), with_lm, with_lodr});
            else model->engine.beam_chunk_host(enc_out, B, Tc, K, bin.data(), bout.data());
        }
        // (only after success: a failed call leaves every stream as it was -- the LM state blocks' halves flip here too)
        nlm.done = true;
        for (int b = 0; b < B; b++) {
            if (nlm.active) nlm.flip(*streams[b]->nlm);
            const float* yp = ypb.empty() ? nullptr : ypb.data() + (size_t)b * K * Tc;
            if (any_hw) streams[b]->hist.apply_out_states(bout.data() + (size_t)b * L.out_ints(), Tc, st_out.data() + (size_t)b * K, yp,
                                                          with_lm ? st_out.data() + (size_t)(B + b) * K : nullptr,
                                                          with_lodr ? st_out.data() + ((size_t)(planes - 1) * B + b) * K : nullptr);
            else streams[b]->hist.apply_out(bout.data() + (size_t)b * L.out_ints(), Tc, yp);
        }
    });
}
int32_t k2hip_beam_stream_num_tokens(const k2hip_beam_stream_t* s) { return s ? (int32_t)s->hist.tokens().size() - 2 : -1; }
int32_t k2hip_beam_stream_get_tokens(const k2hip_beam_stream_t* s, int64_t* tokens, int32_t cap) {
    return guard([&] {
        NEED(s);
        const std::vector<int64_t>& t = s->hist.tokens();
        if ((int)t.size() - 2 > cap) failf(K2HIP_ERR_CAPACITY, "beam stream holds %zu tokens", t.size() - 2);
        if (t.size() > 2) { NEED(tokens); memcpy(tokens, t.data() + 2, sizeof(int64_t) * (t.size() - 2)); }
    });
}
int32_t k2hip_beam_stream_get_timestamps(const k2hip_beam_stream_t* s, int32_t* timestamps, int32_t cap) {
    return guard([&] {
        NEED(s);
        const std::vector<int32_t>& t = s->hist.timestamps();
        if ((int)t.size() > cap) failf(K2HIP_ERR_CAPACITY, "beam stream holds %zu timestamps", t.size());
        if (!t.empty()) { NEED(timestamps); memcpy(timestamps, t.data(), sizeof(int32_t) * t.size()); }
    });
}
int32_t k2hip_beam_stream_get_score(const k2hip_beam_stream_t* s, float* score) {
    return guard([&] {
        NEED(s); NEED(score);
        *score = s->hist.score();
    });
}
int32_t k2hip_beam_stream_num_alternatives(const k2hip_beam_stream_t* s) {
    return s ? (int32_t)s->hist.nbest(s->model->nbest.load()).size() : -1;
}
int32_t k2hip_beam_stream_get_alternative(const k2hip_beam_stream_t* s, int32_t i, int64_t* tokens, int32_t* timestamps, float* token_log_probs,
                                          int32_t cap, int32_t* n, float* score) {
    return guard([&] {
        NEED(s);
        alt_get(s->hist.nbest(s->model->nbest.load()), i, tokens, timestamps, token_log_probs, cap, n, score);
    });
}
int32_t k2hip_beam_stream_get_token_log_probs(const k2hip_beam_stream_t* s, float* out, int32_t cap) {
    if (!s) return guard([&] { NEED(s); });
    return yp_get(s->hist.token_log_probs(), out, cap);
}
// ---- operator level of the streaming CTC prefix beam search -------------------------------------------------------------------------
int32_t k2hip_ctc_prefix_stream_create(k2hip_model_t* model, int32_t beam, int32_t nbest, k2hip_ctc_prefix_stream_t** out) {
    return guard([&] {
        NEED(model); NEED(out);
        *out = nullptr;
        if (!model->engine.model().cfg().ctc)
            failf(K2HIP_ERR_UNSUPPORTED, "ctc prefix stream: model_type '%s' has no CTC head", model->engine.model().cfg().model_type.c_str());
        K2_REQUIRE(beam >= 1 && beam <= kMaxBeam, "ctc prefix stream: beam %d out of range [1,%d]", beam, kMaxBeam);
        K2_REQUIRE(nbest >= 1 && nbest <= beam, "ctc prefix stream: nbest %d out of range [1, beam = %d]", nbest, beam);
        *out = new k2hip_ctc_prefix_stream{model, CtcPrefixHistory(beam, nbest)};
    });
}
int32_t k2hip_ctc_prefix_stream_destroy(k2hip_ctc_prefix_stream_t* s) {
    return guard([&] { delete s; });
}
int32_t k2hip_ctc_prefix_stream_reset(k2hip_ctc_prefix_stream_t* s) {
    return guard([&] {
        NEED(s);
        s->hist.reset();
    });
}
int32_t k2hip_ctc_prefix_stream_set_hotwords(k2hip_ctc_prefix_stream_t* s, const k2hip_hotwords_t* hw) {
    return guard([&] {
        NEED(s);
        K2_REQUIRE(s->hist.frames() == 0, "ctc prefix stream set_hotwords: the stream has searched %lld frames and its prefixes carry states of the "
                   "graph it started with -- reset the stream first", s->hist.frames());
        s->hw = hw ? hw_resident_get(s->model, hw, "ctc prefix stream set_hotwords") : nullptr;
    });
}
int32_t k2hip_ctc_prefix_stream_set_biasing(k2hip_ctc_prefix_stream_t* s, int32_t on) {
    return guard([&] {
        NEED(s);
        K2_REQUIRE(s->hist.frames() == 0, "ctc prefix stream set_biasing: the stream has searched %lld frames and its prefixes carry the states of "
                   "the search it started with -- reset the stream first", s->hist.frames());
        s->biasing = on != 0;
    });
}
int64_t k2hip_ctc_prefix_stream_num_frames(const k2hip_ctc_prefix_stream_t* s) { return s ? (int64_t)s->hist.frames() : -1; }
int32_t k2hip_ctc_prefix_beam_search_chunk(k2hip_model_t* model, k2hip_ctc_prefix_stream_t* const* streams, int32_t B, const float* log_probs, int32_t Tc,
                                           const int32_t* n_frames) {
    return guard([&] {
        NEED(model); NEED(streams); NEED(log_probs);
        if (!model->engine.model().cfg().ctc)
            failf(K2HIP_ERR_UNSUPPORTED, "ctc_prefix_beam_search_chunk: model_type '%s' has no CTC head", model->engine.model().cfg().model_type.c_str());
        K2_REQUIRE(B > 0 && B <= 65535 && Tc >= 1, "ctc_prefix_beam_search_chunk: bad shape B=%d Tc=%d", B, Tc);
        std::vector<const k2hip_ctc_prefix_stream*> seen(streams, streams + B);
        for (int b = 0; b < B; b++) {
            NEED(streams[b]);
            K2_REQUIRE(streams[b]->model == model, "ctc prefix stream %d belongs to another model", b);
            K2_REQUIRE(streams[b]->hist.beam() == streams[0]->hist.beam(), "ctc prefix stream %d has beam %d, stream 0 has %d: one beam per call", b,
                       streams[b]->hist.beam(), streams[0]->hist.beam());
            K2_REQUIRE(!n_frames || (n_frames[b] >= 1 && n_frames[b] <= Tc), "ctc_prefix_beam_search_chunk: stream %d has n_frames = %d outside [1, Tc = %d]", b,
                       n_frames[b], Tc);
        }
        std::sort(seen.begin(), seen.end());
        K2_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "ctc_prefix_beam_search_chunk: the same stream appears twice");
        const int K = streams[0]->hist.beam();
        const CtcPrefixResumeLayout L{K, Tc};
        std::vector<int> bin((size_t)B * L.in_ints()), bout((size_t)B * L.out_ints());
        // biasing is per stream and opt-in: with no biased stream in the call this is the plain call, unchanged
        bool any_bias = false;
        for (int b = 0; b < B; b++) any_bias = any_bias || streams[b]->biasing;
        CtcPrefixBiasCall cpb;
        const CtcPrefixResumeBiasLayout SL{K};
        if (any_bias) {
            {
                EngineLock lk(model->engine);
                cpb.lm_serial = model->lm_serial; cpb.lm_start = model->lm_start; cpb.lm_states = model->lm_states;
            }
            for (int b = 0; b < B; b++)
                if (streams[b]->biasing) CtcPrefixBiasCall::check_lm(streams[b]->hist, cpb.lm_serial, "ctc_prefix_beam_search_chunk", b);
            cpb.stage(B, K);
            for (int b = 0; b < B; b++) cpb.fill(b, K, streams[b]->hist, streams[b]->hw.get(), streams[b]->biasing);
        }
        for (int b = 0; b < B; b++) streams[b]->hist.fill_in(bin.data() + (size_t)b * L.in_ints(), Tc);
        {
            EngineLock lk(model->engine);
            // (this lock covers the launch and k2hip_set_ngram_lm takes it too: the staged LM states still index the tables that are set)
            K2_REQUIRE(!any_bias || model->lm_serial == cpb.lm_serial, "ctc_prefix_beam_search_chunk: k2hip_set_ngram_lm changed the n-gram LM while this "
                                                                        "call was being prepared; call again");
            if (any_bias)
                model->engine.ctc_prefix_chunk_host_bias(log_probs, B, Tc, n_frames, K, bin.data(), bout.data(),
                                                         Engine::CtcPrefixBiasIO{cpb.graphs.data(), cpb.side_in.data(), cpb.side_out.data(), cpb.with_lm()});
            else model->engine.ctc_prefix_chunk_host(log_probs, B, Tc, n_frames, K, bin.data(), bout.data());
        }
        // (only after success, and after every out block has passed its check: a failed call leaves every stream as it was)
        for (int b = 0; b < B; b++) {
            const int nf = n_frames ? n_frames[b] : Tc;
            if (streams[b]->biasing)
                streams[b]->hist.check_out(bout.data() + (size_t)b * L.out_ints(), cpb.side_out.data() + (size_t)b * SL.out_ints(), Tc, nf,
                                           CtcPrefixBiasCall::graph_states(streams[b]->hw.get(), true), cpb.with_lm() ? cpb.lm_states : 0);
            else streams[b]->hist.check_out(bout.data() + (size_t)b * L.out_ints(), Tc, nf);
        }
        for (int b = 0; b < B; b++) {
            const int nf = n_frames ? n_frames[b] : Tc;
            if (streams[b]->biasing) streams[b]->hist.apply_out(bout.data() + (size_t)b * L.out_ints(), cpb.side_out.data() + (size_t)b * SL.out_ints(), Tc, nf);
            else streams[b]->hist.apply_out(bout.data() + (size_t)b * L.out_ints(), Tc, nf);
        }
    });
}
int32_t k2hip_ctc_prefix_stream_num_tokens(const k2hip_ctc_prefix_stream_t* s) { return s ? (int32_t)s->hist.tokens().size() : -1; }
int32_t k2hip_ctc_prefix_stream_get_tokens(const k2hip_ctc_prefix_stream_t* s, int64_t* tokens, int32_t cap) {
    return guard([&] {
        NEED(s);
        const std::vector<int64_t>& t = s->hist.tokens();
        if ((int)t.size() > cap) failf(K2HIP_ERR_CAPACITY, "ctc prefix stream holds %zu tokens", t.size());
        if (!t.empty()) { NEED(tokens); memcpy(tokens, t.data(), sizeof(int64_t) * t.size()); }
    });
}
int32_t k2hip_ctc_prefix_stream_get_timestamps(const k2hip_ctc_prefix_stream_t* s, int32_t* timestamps, int32_t cap) {
    return guard([&] {
        NEED(s);
        const std::vector<int32_t>& t = s->hist.timestamps();
        if ((int)t.size() > cap) failf(K2HIP_ERR_CAPACITY, "ctc prefix stream holds %zu timestamps", t.size());
        if (!t.empty()) { NEED(timestamps); memcpy(timestamps, t.data(), sizeof(int32_t) * t.size()); }
    });
}
int32_t k2hip_ctc_prefix_stream_get_token_log_probs(const k2hip_ctc_prefix_stream_t* s, float* out, int32_t cap) {
    if (!s) return guard([&] { NEED(s); });
    return yp_get(s->hist.token_log_probs(), out, cap);
}
int32_t k2hip_ctc_prefix_stream_get_score(const k2hip_ctc_prefix_stream_t* s, float* score) {
    return guard([&] {
        NEED(s); NEED(score);
        *score = s->hist.score();
    });
}
int32_t k2hip_ctc_prefix_stream_num_alternatives(const k2hip_ctc_prefix_stream_t* s) {
    return s ? (int32_t)s->hist.nbest(s->hist.nbest_limit()).size() : -1;
}
int32_t k2hip_ctc_prefix_stream_get_alternative(const k2hip_ctc_prefix_stream_t* s, int32_t i, int64_t* tokens, int32_t* timestamps, float* token_log_probs,
                                                int32_t cap, int32_t* n, float* score) {
    return guard([&] {
        NEED(s);
        alt_get(s->hist.nbest(s->hist.nbest_limit()), i, tokens, timestamps, token_log_probs, cap, n, score);
    });
}
// (a stream that has not decoded a chunk yet is in the start state: one empty alternative, score 0)
static std::vector<BeamAlt> online_alts(const k2hip_online_stream* s) {
    if (s->cp_beam > 0) return s->cprefix ? s->cprefix->nbest(s->cp_nbest) : std::vector<BeamAlt>(1);
    K2_REQUIRE(s->method != 0, "the stream decodes with greedy_search: it has no alternatives");
    return s->method > 0 ? s->beam->nbest(s->model->nbest.load()) : std::vector<BeamAlt>(1);
}
int32_t k2hip_online_stream_num_alternatives(const k2hip_online_stream_t* s) {
    int32_t count = 0;
    const int32_t rc = guard([&] {
        NEED(s);
        count = (int32_t)online_alts(s).size();
    });
    return rc < 0 ? rc : count;
}
int32_t k2hip_online_stream_get_alternative(const k2hip_online_stream_t* s, int32_t i, int64_t* tokens, int32_t* timestamps,
                                            float* token_log_probs, int32_t cap, int32_t* n, float* score) {
    return guard([&] {
        NEED(s);
        alt_get(online_alts(s), i, tokens, timestamps, token_log_probs, cap, n, score);
    });
}
int32_t k2hip_online_stream_get_token_log_probs(const k2hip_online_stream_t* s, float* out, int32_t cap) {
    if (!s) return guard([&] { NEED(s); });
    static const std::vector<float> none;
    if (s->cp_beam > 0) return yp_get(s->cprefix ? s->cprefix->token_log_probs() : none, out, cap);
    if (s->method == 0) return guard([&] { K2_REQUIRE(false, "the stream decodes with greedy_search: it keeps no token log-probs"); });
    return yp_get(s->method > 0 ? s->beam->token_log_probs() : none, out, cap);
}
int32_t k2hip_online_stream_get_hyp(const k2hip_online_stream_t* s, int64_t* hyp2) {
    return guard([&] {
        NEED(s); NEED(hyp2);
        hyp2[0] = s->hyp[0];
        hyp2[1] = s->hyp[1];
    });
}
int32_t k2hip_online_stream_state(k2hip_online_stream_t* s, int32_t layer, int32_t kind, float* out, int64_t cap, int64_t* n) {
    return guard([&] {
        NEED(s); NEED(n);
        EngineLock lk(s->model->engine);
        s->model->engine.online_read_state(s->slot, layer, kind, s->chunks_done, out, cap, n);
    });
}

// hotword graphs uploaded for this model's streams so far, and how many are resident now (k2hip_debug.h)
int32_t k2hip_debug_stream_hotword_uploads(k2hip_model_t* model, int32_t* uploads, int32_t* resident) {
    return guard([&] {
        NEED(model); NEED(uploads); NEED(resident);
        std::lock_guard<std::mutex> g(g_hw_mu);
        *uploads = model->hw_uploads;
        int n = 0;
        for (auto& kv : model->hw_cache) n += !kv.second.expired();
        *resident = n;
    });
}
int32_t k2hip_debug_beam_launch_counts(int64_t* plain, int64_t* hotwords) {
    return guard([&] {
        NEED(plain); NEED(hotwords);
        long long p = 0, h = 0;
        beam_launch_counts(&p, &h);
        *plain = p;
        *hotwords = h;
    });
}
// one-part repeats of the vocabulary-parallel search since the model was created (test / monitoring hook: include/k2hip_debug.h)
int32_t k2hip_debug_search_retries(k2hip_model_t* model, int32_t* n) {
    return guard([&] {
        NEED(model); NEED(n);
        EngineLock lk(model->engine);
        *n = model->engine.search_retries();
    });
}
int32_t k2hip_debug_beam_trace(k2hip_model_t* model, int32_t* trace, int64_t cap_words, int32_t* B, int32_t* Tprime, int32_t* beam) {
    return guard([&] {
        NEED(model); NEED(B); NEED(Tprime); NEED(beam);
        EngineLock lk(model->engine);
        int b = 0, tp = 0, k = 0;
        const std::vector<int>& t = model->engine.last_beam_trace(&b, &tp, &k);
        K2_REQUIRE(!t.empty(), "beam trace: no traced beam search on record (set K2HIP_BEAM_TRACE=1 before the call)");
        *B = b; *Tprime = tp; *beam = k;
        if (!trace) return;
        if ((int64_t)t.size() > cap_words) failf(K2HIP_ERR_CAPACITY, "beam trace: %zu words exceed capacity %lld", t.size(), (long long)cap_words);
        memcpy(trace, t.data(), sizeof(int) * t.size());
    });
}
// test hook (include/k2hip_debug.h): the all-contexts decoder table against the decoder itself on sampled contexts
int32_t k2hip_debug_decoder_table_check(k2hip_model_t* model, int32_t n_samples, uint32_t seed,
                                                                                int64_t* rows, int64_t* mismatched) {
    return guard([&] {
        NEED(model); NEED(rows); NEED(mismatched);
        K2_REQUIRE(n_samples >= 0 && n_samples <= 65536, "decoder table check: %d samples", n_samples);
        EngineLock lk(model->engine);
        long long r = 0, m = 0;
        model->engine.decoder_table_check(n_samples, seed, &r, &m);
        *rows = r;
        *mismatched = m;
    });
}
// test hook (include/k2hip_debug.h): mark a stream as if a chunk step over it had failed on the device
int32_t k2hip_debug_poison_stream(k2hip_online_stream_t* s) {
    return guard([&] {
        NEED(s);
        s->poisoned = true;
    });
}

// test hook (include/k2hip_debug.h): does the stream's device mirror of its feature FIFO hold the FIFO right now?
int32_t k2hip_debug_stream_mirrored(const k2hip_online_stream_t* s, int32_t* ok) {
    return guard([&] {
        NEED(s); NEED(ok);
        *ok = s->mir_ok ? 1 : 0;
    });
}

// ---- tuning hook (include/k2hip_debug.h): time one GEMM shape/config on random data
int32_t k2hip_debug_set_switch(const char* env_name, int32_t value) {
    return guard([&] {
        NEED(env_name);
        tunables_init_from_env();  // so that a later model creation does not overwrite what is set here
        if (!tunables_set(env_name, value)) failf(K2HIP_ERR_INVALID, "unknown switch '%s'", env_name);
    });
}
// the offline conv module's fused form for a shape (gemm_plan.cpp glu_dwconv_pipe_entry): host only, no model, no device
int32_t k2hip_debug_conv_fused_plan(int32_t B, int32_t T, int32_t D, int32_t K, int32_t streaming, int32_t* entry) {
    return guard([&] {
        NEED(entry);
        tunables_init_from_env();
        *entry = glu_dwconv_pipe_entry(B, T, D, K, streaming != 0);
    });
}
int32_t k2hip_debug_gemm(k2hip_model_t* model, int32_t M, int32_t N, int32_t K,
                                                                 int32_t act, int32_t with_res, int32_t cfg, int32_t iters, float* ms) {
    return guard([&] {
        NEED(model); NEED(ms);
        EngineLock lk(model->engine);
        *ms = model->engine.debug_gemm(M, N, K, act, with_res != 0, iters, cfg, nullptr);
    });
}
// the same, and max_err = largest |difference| from the register-staged kernel on the same operands
int32_t k2hip_debug_gemm_check(k2hip_model_t* model, int32_t M, int32_t N, int32_t K,
                                                                       int32_t act, int32_t with_res, int32_t cfg, int32_t iters, float* ms,
                                                                       float* max_err) {
    return guard([&] {
        NEED(model); NEED(ms); NEED(max_err);
        EngineLock lk(model->engine);
        *ms = model->engine.debug_gemm(M, N, K, act, with_res != 0, iters, cfg, max_err);
    });
}

int32_t k2hip_debug_gemm_run(k2hip_model_t* model, const float* A, const float* W, const float* bias, const float* res, float* C, int32_t M,
                             int32_t N, int32_t K, int32_t act, int32_t glu, int32_t glu_cols, int32_t cfg) {
    return guard([&] {
        NEED(model); NEED(A); NEED(W); NEED(C);
        EngineLock lk(model->engine);
        model->engine.debug_gemm_host(A, W, bias, res, C, M, N, K, act, glu, glu_cols, cfg);
    });
}

int32_t k2hip_debug_op_run(k2hip_model_t* model, const char* op, const int64_t* iargs, int32_t n_iargs, void* const* bufs,
                           const int64_t* buf_bytes, int32_t n_bufs, uint32_t out_mask) {
    return guard([&] {
        NEED(model); NEED(op);
        if (!Engine::debug_op) failf(K2HIP_ERR_UNSUPPORTED, "debug_op_run: this build has no kernels");
        EngineLock lk(model->engine);
        (model->engine.*Engine::debug_op)(op, iargs, n_iargs, bufs, buf_bytes, n_bufs, out_mask);
    });
}

int32_t k2hip_debug_gemm_trace(k2hip_model_t* model, int32_t M, int32_t N, int32_t K, int32_t act,
                                                                       int32_t with_res, int32_t cfg, unsigned long long* out, int64_t cap,
                                                                       int32_t* n_wg, int32_t* n_waves) {
    return guard([&] {
        NEED(model); NEED(out); NEED(n_wg); NEED(n_waves);
        EngineLock lk(model->engine);
        model->engine.debug_gemm_trace(M, N, K, act, with_res != 0, cfg, out, cap, n_wg, n_waves);
    });
}

// ---- OfflineStream ---------------------------------------------------------------
int32_t k2hip_offline_stream_create(k2hip_model_t* model, k2hip_offline_stream_t** out) {
    return guard([&] {
        NEED(model); NEED(out);
        auto* s = new k2hip_offline_stream();
        s->model = model;
        s->tokens = {K2HIP_BLANK_ID, K2HIP_BLANK_ID};  // OfflineStream.cs:34
        *out = s;
    });
}
int32_t k2hip_offline_stream_destroy(k2hip_offline_stream_t* s) {
    return guard([&] {
        if (s && s->wav.capacity() > 0) {   // the buffer goes back to the model's pool (touched pages: no first-touch faults next time)
            std::lock_guard<std::mutex> lk(s->model->wav_mu);
            if (s->model->wav_pool.size() < k2hip_model::kPoolMax) {
                s->wav.clear();
                s->model->wav_pool.push_back(std::move(s->wav));
            }
        }
        delete s;
    });
}
// frames the stream's unmaterialised samples will add to Speech
// samples at the model's rate that the stream's queue gives: the queue itself, or what the resampler makes of it
static int64_t offline_queued(const k2hip_offline_stream* s) {
    return s->rs ? s->rs->num_out(s->rs_x0 + (int64_t)s->wav.size()) - s->rs_k0 : (int64_t)s->wav.size();
}
static int64_t offline_pending_frames(const k2hip_offline_stream* s) {
    return s->wav.empty() ? 0 : s->model->engine.fbank_num_frames(offline_queued(s));
}
// nf frames of the queue are spoken for: the samples behind the last whole frame shift stay queued -- of a resampling stream, the
// input behind it AND behind what the resampler still reads for the outputs to come
static void offline_erase_frames(k2hip_offline_stream* s, int64_t nf) {
    const int64_t used = nf * s->model->engine.model().cfg().fbank.frame_shift;
    if (!s->rs) {
        s->wav.erase_front((size_t)used);
        return;
    }
    s->rs_k0 += used;
    const int64_t keep = std::min(s->rs->keep_from(s->rs_k0), s->rs_x0 + (int64_t)s->wav.size());
    s->wav.erase_front((size_t)(keep - s->rs_x0));
    s->rs_x0 = keep;
}
// the batch's resampling streams named to the engine for one from-samples call (Engine::set_wave_srcs); made under the engine's lock
struct WaveSrcScope {
    Engine& e;
    std::vector<Engine::WaveSrc> w;
    WaveSrcScope(Engine& eng, k2hip_offline_stream* const* streams, int B) : e(eng), w((size_t)B) {
        bool any = false;
        for (int b = 0; b < B; b++) {
            w[(size_t)b] = Engine::WaveSrc{streams[b]->rs, streams[b]->rs_x0, streams[b]->rs_k0};
            any = any || streams[b]->rs;
        }
        if (any) e.set_wave_srcs(w.data());
    }
    ~WaveSrcScope() { e.set_wave_srcs(nullptr); }
};
// run the fbank of the stream's unmaterialised samples now and append the frames to Speech; the samples behind the last whole frame
// shift stay queued (the streaming framing of an OnlineFbank)
static void offline_materialize(k2hip_offline_stream* s) {
    Engine& e = s->model->engine;
    const Config& c = e.model().cfg();
    const int64_t nf = offline_pending_frames(s);
    if (nf <= 0) return;
    const size_t old = s->speech.size();
    s->speech.resize(old + (size_t)nf * c.feat);
    try {
        int64_t got = 0;
        EngineLock lk(e);
        if (s->rs) {
            std::vector<float> y((size_t)offline_queued(s));
            const Engine::ResampleJob job{s->rs, s->wav.data(), (int64_t)s->wav.size(), nullptr, 0, s->rs_x0, s->rs_k0, (int64_t)y.size(), y.data()};
            e.resample_host(&job, 1);
            e.fbank_host(y.data(), (int64_t)y.size(), s->speech.data() + old, nf, &got);
        } else {
            e.fbank_host(s->wav.data(), (int64_t)s->wav.size(), s->speech.data() + old, nf, &got);
        }
    } catch (...) {
        s->speech.resize(old);
        throw;
    }
    offline_erase_frames(s, nf);
}
// OfflineStream.AddSamples (:43-57): the samples are queued; their frames count in SpeechLength at once and are computed when
// somebody needs them (GetResults: on the device, for the whole batch in one launch)
static void offline_add(k2hip_offline_stream* s, const float* samples, int64_t n);
int32_t k2hip_offline_stream_accept_samples(k2hip_offline_stream_t* s, const float* samples, int64_t n) {
    return guard([&] {
        NEED(s);
        if (n > 0) NEED(samples);
        if (n <= 0) return;
        const int own = s->model->engine.model().cfg().fbank.sample_rate;
        K2_REQUIRE(!s->rs, "accept_samples: the stream resamples from %d Hz (accept_waveform), these samples are at the model's %d Hz", s->rate, own);
        s->rate = own;
        offline_add(s, samples, n);
    });
}
// a stream fed at another rate queues its raw samples as any other does: nothing is launched, no lock on the model is taken
int32_t k2hip_offline_stream_accept_waveform(k2hip_offline_stream_t* s, int32_t sample_rate, const float* samples, int64_t n) {
    return guard([&] {
        NEED(s);
        if (n > 0) NEED(samples);
        const ResamplePlan* p = take_rate(s->model, &s->rate, &s->rs, sample_rate, "accept_waveform");
        if (n <= 0) return;
        K2_REQUIRE(!p || s->rs_x0 + (int64_t)s->wav.size() + n < kResampleMaxInput, "accept_waveform: more than 2^36 samples in one stream");
        offline_add(s, samples, n);
    });
}
static void offline_add(k2hip_offline_stream* s, const float* samples, int64_t n) {
    if (s->wav.capacity() == 0) {   // first samples of the stream: a buffer of the model's pool that is large enough, if there is one
        std::lock_guard<std::mutex> lk(s->model->wav_mu);
        auto& pool = s->model->wav_pool;
        for (size_t i = pool.size(); i-- > 0;)
            if (pool[i].capacity() >= (size_t)n) {
                s->wav = std::move(pool[i]);
                pool.erase(pool.begin() + (long)i);
                break;
            }
    }
    s->wav.append(s->model->engine, samples, (size_t)n);
}
int64_t k2hip_offline_stream_speech_length(const k2hip_offline_stream_t* s) {
    return s ? (int64_t)s->speech.size() + offline_pending_frames(s) * s->model->engine.model().cfg().feat : -1;
}
int32_t k2hip_offline_stream_get_speech(const k2hip_offline_stream_t* s_, float* out, int64_t cap) {
    return guard([&] {
        NEED(s_);
        k2hip_offline_stream* s = const_cast<k2hip_offline_stream*>(s_);   // (materialising the frames does not change what the stream IS)
        offline_materialize(s);
        if ((int64_t)s->speech.size() > cap) failf(K2HIP_ERR_CAPACITY, "speech has %zu floats", s->speech.size());
        if (!s->speech.empty()) {
            NEED(out);
            memcpy(out, s->speech.data(), sizeof(float) * s->speech.size());
        }
    });
}

// OfflineStream.RemoveSamples (:58-68) after a search that consumed the stream's samples straight from `wav`: Speech = null when
// Tokens.Count > Context_size; otherwise the reference keeps the features -- they are materialised then (a rare path: one stream
// that emitted nothing).  Either way the samples behind the last whole frame shift stay queued.
static void offline_consume(k2hip_offline_stream* s, int ctx) {
    if ((int)s->tokens.size() > ctx) {
        const int64_t nf = offline_pending_frames(s);
        if (nf > 0) offline_erase_frames(s, nf);
        s->speech.clear();
        s->speech.shrink_to_fit();
    } else {
        offline_materialize(s);
    }
}

// OfflineRecognizer.GetResults -> ForwardBatchGreedySearch (:85-91, :189-303)
int32_t k2hip_offline_recognizer_get_results(k2hip_model_t* model, k2hip_offline_stream_t* const* streams, int32_t B) {
    return guard([&] {
        NEED(model); NEED(streams);
        K2_REQUIRE(B > 0, "GetResults: empty stream list");
        Engine& e = model->engine;
        const Config& c = e.model().cfg();
        bool from_samples = true;   // no stream holds materialised features: the whole batch goes samples -> tokens on the device
        for (int b = 0; b < B; b++) {
            NEED(streams[b]);
            K2_REQUIRE(streams[b]->model == model, "stream %d belongs to another model", b);
            from_samples = from_samples && streams[b]->speech.empty() && offline_pending_frames(streams[b]) > 0;
        }
        {   // one stream twice in the list would be decoded twice and have its samples consumed twice
            std::vector<const k2hip_offline_stream*> seen(streams, streams + B);
            std::sort(seen.begin(), seen.end());
            K2_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "GetResults: the same stream appears twice in the list");
        }
        std::vector<const float*> ptrs(B);
        std::vector<int64_t> nfl(B);
        int64_t mx = 0;
        if (!from_samples)
            for (int b = 0; b < B; b++) offline_materialize(streams[b]);
        for (int b = 0; b < B; b++) {
            ptrs[b] = from_samples ? streams[b]->wav.data() : streams[b]->speech.data();
            nfl[b] = from_samples ? (int64_t)streams[b]->wav.size() : (int64_t)streams[b]->speech.size();
            mx = std::max(mx, from_samples ? offline_pending_frames(streams[b]) * c.feat : nfl[b]);
        }
        int T = (int)((mx + 80 * 19) / c.feat);
        int max_tokens = std::max(1, e.encoder_out_frames(T));
        std::vector<int64_t> tok((size_t)B * max_tokens);
        std::vector<int32_t> ts((size_t)B * max_tokens), n(B);
        for (int b = 0; b < B; b++) streams[b]->alts.assign(1, BeamAlt{});   // (a failed call leaves the start state)
        {
            EngineLock lk(e);
            WaveSrcScope ws(e, streams, B);
            K2_REQUIRE(e.nbest() == 0 || e.beam() > 0 || e.ctc_prefix() > 0, "GetResults: the model keeps %d alternatives (k2hip_set_nbest) but decodes with "
                       "greedy_search, which has none", e.nbest());
            if (from_samples) e.offline_greedy_samples(ptrs.data(), nfl.data(), B, tok.data(), ts.data(), n.data(), max_tokens, false, /*pinned_src=*/true);
            else e.offline_greedy_feats(ptrs.data(), nfl.data(), B, false, tok.data(), ts.data(), n.data(), max_tokens);
            const Engine::NbestHost& h = e.last_nbest();
            // (never one silent result where a list was asked for)
            K2_REQUIRE(e.nbest() == 0 || (h.B == B && h.N == e.nbest()), "internal: GetResults ran with %d alternatives asked for and the search kept no list",
                       e.nbest());
            if (e.nbest() > 0)
                for (int b = 0; b < B; b++) {
                    streams[b]->alts.clear();
                    for (int i = 0; i < h.n_hyps[(size_t)b]; i++) streams[b]->alts.push_back(alt_of(h, b, i));
                }
            // (an active fusion has put the LM's terms into the transducer search's scores already: rescoring would count it twice)
            const bool fused = !c.ctc && e.beam() > 0 && e.rnn_lm_fusion_active();
            if (!fused && e.nbest() > 1 && model->rnn_lm && model->rnn_scale > 0.f && (c.ctc ? e.ctc_prefix() > 0 : e.beam() > 0))
                try {
                    rnn_lm_rescore(model, streams, B, max_tokens, tok.data(), ts.data(), n.data());
                } catch (...) {   // (a failed call leaves the start state)
                    for (int b = 0; b < B; b++) streams[b]->alts.assign(1, BeamAlt{});
                    throw;
                }
        }
        auto remove_samples = [&](k2hip_offline_stream* s) {   // RemoveSamples (:294 / :418, OfflineStream.cs:58-68)
            if (from_samples) {
                offline_consume(s, c.ctx);
            } else if ((int)s->tokens.size() > c.ctx) {
                s->speech.clear();
                s->speech.shrink_to_fit();
            }
        };
        if (c.ctc) {
            // ForwardBatchGreedySearchCTC (:366-424): new symbols are appended to the stream's OWN lists (Tokens starts as
            // [blank, blank], OfflineStream.cs:34), timestamps carry FrameOffset, NumTrailingBlank accumulates
            const std::vector<int>&trail = e.last_trail(), &any = e.last_any();
            for (int b = 0; b < B; b++) {
                k2hip_offline_stream* s = streams[b];
                for (int k = 0; k < n[b]; k++) {
                    s->tokens.push_back(tok[(size_t)b * max_tokens + k]);
                    s->timestamps.push_back(ts[(size_t)b * max_tokens + k] + s->frame_offset);
                }
                s->num_trailing_blank = any[b] ? trail[b] : s->num_trailing_blank + trail[b];
                remove_samples(s);
            }
            return;
        }
        for (int b = 0; b < B; b++) {
            k2hip_offline_stream* s = streams[b];
            // tokens[m] / timestamps[m] are seeded with 2*B blanks / zeros (:250-267)
            s->tokens.assign((size_t)2 * B, K2HIP_BLANK_ID);
            s->tokens.insert(s->tokens.end(), tok.begin() + (size_t)b * max_tokens, tok.begin() + (size_t)b * max_tokens + n[b]);
            s->timestamps.insert(s->timestamps.end(), (size_t)2 * B, 0);  // Timestamps.AddRange (:293)
            s->timestamps.insert(s->timestamps.end(), ts.begin() + (size_t)b * max_tokens, ts.begin() + (size_t)b * max_tokens + n[b]);
            remove_samples(s);
        }
    });
}
// OfflineRecognizer.GetResult -> ForwardGreedySearch (:77-83, :93-187)
int32_t k2hip_offline_recognizer_get_result(k2hip_model_t* model, k2hip_offline_stream_t* s) {
    return guard([&] {
        NEED(model); NEED(s);
        K2_REQUIRE(s->model == model, "stream belongs to another model");
        Engine& e = model->engine;
        const Config& c = e.model().cfg();
        const bool from_samples = s->speech.empty() && offline_pending_frames(s) > 0;
        const int64_t n_fl = from_samples ? offline_pending_frames(s) * c.feat : (int64_t)s->speech.size();
        int T = (int)((n_fl + 80 * 19) / c.feat);
        int max_tokens = std::max(1, e.encoder_out_frames(T));
        std::vector<int64_t> tok(max_tokens);
        std::vector<int32_t> ts(max_tokens);
        int32_t n = 0;
        const float* p[1] = {from_samples ? s->wav.data() : s->speech.data()};
        int64_t nfl[1] = {from_samples ? (int64_t)s->wav.size() : (int64_t)s->speech.size()};
        s->alts.assign(1, BeamAlt{});
        {
            EngineLock lk(e);
            WaveSrcScope ws(e, &s, 1);
            // (the single-stream path is the reference's greedy loop whatever the decoding method: it has no alternatives)
            K2_REQUIRE(e.nbest() == 0, "GetResult: the single-stream path is greedy search and the model keeps %d alternatives "
                       "(k2hip_set_nbest) -- use GetResults", e.nbest());
            if (from_samples) e.offline_greedy_samples(p, nfl, 1, tok.data(), ts.data(), &n, max_tokens, true, /*pinned_src=*/true);
            else e.offline_greedy_feats(p, nfl, 1, true, tok.data(), ts.data(), &n, max_tokens);
        }
        s->tokens = {-1, K2HIP_BLANK_ID};  // hypList (:115-117, :180); the CTC single path seeds the same pair (:318-320)
        s->tokens.insert(s->tokens.end(), tok.begin(), tok.begin() + n);
        s->timestamps.insert(s->timestamps.end(), ts.begin(), ts.begin() + n);  // (:181; CTC :355 with frameOffset = 0)
        if (c.ctc) s->num_trailing_blank = e.last_any()[0] ? e.last_trail()[0] : e.last_trail()[0];  // local counter from 0 (:316,:354)
        // (the single paths never call RemoveSamples, :93-187 / :305-364: Speech stays -- materialised now if the search took the samples)
        if (from_samples) offline_materialize(s);
    });
}
int32_t k2hip_offline_stream_num_alternatives(const k2hip_offline_stream_t* s) { return s ? (int32_t)s->alts.size() : -1; }
int32_t k2hip_offline_stream_get_alternative(const k2hip_offline_stream_t* s, int32_t i, int64_t* tokens, int32_t* timestamps,
                                             float* token_log_probs, int32_t cap, int32_t* n, float* score) {
    return guard([&] {
        NEED(s);
        alt_get(s->alts, i, tokens, timestamps, token_log_probs, cap, n, score);
    });
}
int32_t k2hip_offline_stream_get_token_log_probs(const k2hip_offline_stream_t* s, float* out, int32_t cap) {
    if (!s) return guard([&] { NEED(s); });
    return yp_get(s->alts[0].token_log_probs, out, cap);
}
int32_t k2hip_offline_stream_num_tokens(const k2hip_offline_stream_t* s) { return s ? (int32_t)s->tokens.size() : -1; }
int32_t k2hip_offline_stream_num_timestamps(const k2hip_offline_stream_t* s) { return s ? (int32_t)s->timestamps.size() : -1; }
int32_t k2hip_offline_stream_get_tokens(const k2hip_offline_stream_t* s, int64_t* tokens, int32_t cap) {
    return guard([&] {
        NEED(s);
        if ((int)s->tokens.size() > cap) failf(K2HIP_ERR_CAPACITY, "stream holds %zu tokens", s->tokens.size());
        if (!s->tokens.empty()) {
            NEED(tokens);
            memcpy(tokens, s->tokens.data(), sizeof(int64_t) * s->tokens.size());
        }
    });
}
int32_t k2hip_offline_stream_get_timestamps(const k2hip_offline_stream_t* s, int32_t* timestamps, int32_t cap) {
    return guard([&] {
        NEED(s);
        if ((int)s->timestamps.size() > cap) failf(K2HIP_ERR_CAPACITY, "stream holds %zu timestamps", s->timestamps.size());
        if (!s->timestamps.empty()) {
            NEED(timestamps);
            memcpy(timestamps, s->timestamps.data(), sizeof(int32_t) * s->timestamps.size());
        }
    });
}

}  // extern "C"

// ---- voice activity detection and long recordings (include/k2hip.h; vad_ref.h, vad.hip, vad_engine.cpp) ---------------------------
// One stream of the detector.  `st` is vad_ref.h's carried state, held on the host and riding in every call's upload and download;
// `segs` the reported segments not popped yet.  Samples: `remainder` holds those behind the last whole frame shift, as an online
// stream's does; at another rate the resampler's carried input and counts (resample_ref.h's state) sit in front of it.
struct k2hip_vad_stream {
    k2hip_model* model = nullptr;   // null: a reference stream of the test hooks (k2hip_debug_vad_ref_stream_create)
    int num_bins = 0;
    k2hip_vad_config cfg{};
    VadState st;
    std::vector<VadSeg> segs;
    std::vector<float> remainder;
    int rate = 0;   // fixed by the stream's first samples until a reset or flush (0: none yet)
    std::vector<float> rs_tail;
    int64_t rs_n_in = 0, rs_n_out = 0;
    void restart() {   // what a flush and a reset share
        st = VadState();
        remainder.clear();
        rate = 0;
        rs_tail.clear();
        rs_n_in = rs_n_out = 0;
    }
};
struct k2hip_long_result {
    std::vector<Engine::LongSegment> segs;
};

extern "C" {

int32_t k2hip_vad_default_config(const k2hip_model_t* model, k2hip_vad_config* cfg) {
    return guard([&] {
        NEED(model); NEED(cfg);
        const Config& c = model->engine.model().cfg();
        vad_default_config(c.fbank.sample_rate, c.feat, c.fbank.low_freq, c.fbank.high_freq, cfg);
    });
}
int32_t k2hip_vad_stream_create(k2hip_model_t* model, const k2hip_vad_config* cfg, k2hip_vad_stream_t** out) {
    return guard([&] {
        NEED(model); NEED(cfg); NEED(out);
        *out = nullptr;
        vad_check_config(*cfg, model->engine.model().cfg().feat);
        auto s = std::make_unique<k2hip_vad_stream>();
        s->model = model;
        s->num_bins = model->engine.model().cfg().feat;
        s->cfg = *cfg;
        *out = s.release();
    });
}
int32_t k2hip_vad_stream_destroy(k2hip_vad_stream_t* s) {
    return guard([&] { delete s; });
}
int32_t k2hip_vad_stream_reset(k2hip_vad_stream_t* s) {
    return guard([&] {
        NEED(s);
        s->restart();
        s->segs.clear();
    });
}
int32_t k2hip_vad_stream_flush(k2hip_vad_stream_t* s) {
    return guard([&] {
        NEED(s);
        vad_ref_flush(s->cfg, s->st, &s->segs);
        s->restart();
    });
}
int32_t k2hip_vad_accept_features_batch(k2hip_model_t* model, k2hip_vad_stream_t* const* streams, const float* const* feats, const int64_t* n_frames,
                                        int32_t B) {
    return guard([&] {
        NEED(model); NEED(streams); NEED(feats); NEED(n_frames);
        K2_REQUIRE(B > 0, "vad_accept_features_batch: empty list");
        std::vector<Engine::VadJob> jobs((size_t)B);
        for (int b = 0; b < B; b++) {
            NEED(streams[b]);
            K2_REQUIRE(streams[b]->model == model, "vad_accept_features_batch: stream %d belongs to another model", b);
            K2_REQUIRE(n_frames[b] >= 0, "vad_accept_features_batch: stream %d: %lld frames", b, (long long)n_frames[b]);
            if (n_frames[b] > 0) NEED(feats[b]);
            K2_REQUIRE(streams[b]->remainder.empty() && !streams[b]->rs_n_in, "vad_accept_features_batch: stream %d holds samples short of a frame "
                       "(accept_samples): features and samples do not mix between resets", b);
            jobs[(size_t)b].cfg = &streams[b]->cfg;
            jobs[(size_t)b].st = &streams[b]->st;
            jobs[(size_t)b].segs = &streams[b]->segs;
            jobs[(size_t)b].feats = feats[b];
            jobs[(size_t)b].n = n_frames[b];
        }
        {
            std::vector<const k2hip_vad_stream*> seen(streams, streams + B);
            std::sort(seen.begin(), seen.end());
            K2_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "vad_accept_features_batch: the same stream appears twice in the list");
        }
        EngineLock lk(model->engine);
        model->engine.vad_host(jobs.data(), B, false);
    });
}
int32_t k2hip_vad_accept_samples_batch(k2hip_model_t* model, k2hip_vad_stream_t* const* streams, int32_t sample_rate, const float* const* samples,
                                       const int64_t* n, int32_t B) {
    return guard([&] {
        NEED(model); NEED(streams); NEED(samples); NEED(n);
        K2_REQUIRE(B > 0, "vad_accept_samples_batch: empty list");
        Engine& e = model->engine;
        const Config& c = e.model().cfg();
        const ResamplePlan* plan = model_resample_plan(model, sample_rate);   // (a rate that is refused is refused before any stream moves)
        for (int b = 0; b < B; b++) {
            NEED(streams[b]);
            K2_REQUIRE(streams[b]->model == model, "vad_accept_samples_batch: stream %d belongs to another model", b);
            K2_REQUIRE(n[b] >= 0, "vad_accept_samples_batch: stream %d: %lld samples", b, (long long)n[b]);
            if (n[b] > 0) NEED(samples[b]);
            K2_REQUIRE(streams[b]->rate == 0 || streams[b]->rate == sample_rate, "vad_accept_samples_batch: stream %d takes samples at %d Hz, these are at "
                       "%d Hz (the model's: %d Hz)", b, streams[b]->rate, sample_rate, c.fbank.sample_rate);
            K2_REQUIRE(streams[b]->rs_n_in + n[b] < kResampleMaxInput, "vad_accept_samples_batch: more than 2^36 samples in stream %d", b);
        }
        {
            std::vector<const k2hip_vad_stream*> seen(streams, streams + B);
            std::sort(seen.begin(), seen.end());
            K2_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "vad_accept_samples_batch: the same stream appears twice in the list");
        }
        // at another rate: all streams through the resampler in one launch; the outputs are this call's samples at the model's rate
        std::vector<std::vector<float>> conv((size_t)B);
        EngineLock lk(e);
        if (plan) {
            std::vector<Engine::ResampleJob> rj;
            for (int b = 0; b < B; b++) {
                k2hip_vad_stream* s = streams[b];
                conv[(size_t)b].resize((size_t)(plan->num_out(s->rs_n_in + n[b]) - s->rs_n_out));
                if (!conv[(size_t)b].empty())
                    rj.push_back(Engine::ResampleJob{plan, s->rs_tail.data(), (int64_t)s->rs_tail.size(), samples[b], n[b], s->rs_n_in - (int64_t)s->rs_tail.size(),
                                                     s->rs_n_out, (int64_t)conv[(size_t)b].size(), conv[(size_t)b].data()});
            }
            if (!rj.empty()) e.resample_host(rj.data(), (int)rj.size());
        }
        std::vector<Engine::VadJob> jobs((size_t)B);
        for (int b = 0; b < B; b++) {
            k2hip_vad_stream* s = streams[b];
            Engine::VadJob& j = jobs[(size_t)b];
            j.cfg = &s->cfg; j.st = &s->st; j.segs = &s->segs;
            j.head = s->remainder.data(); j.n_head = (int64_t)s->remainder.size();
            j.tail = plan ? conv[(size_t)b].data() : samples[b];
            j.n_tail = plan ? (int64_t)conv[(size_t)b].size() : n[b];
        }
        e.vad_host(jobs.data(), B, true);
        // the call has succeeded: the streams' sample bookkeeping moves
        for (int b = 0; b < B; b++) {
            k2hip_vad_stream* s = streams[b];
            const Engine::VadJob& j = jobs[(size_t)b];
            if (n[b] > 0) s->rate = sample_rate;
            if (plan && n[b] > 0) {
                const int64_t x0 = s->rs_n_in - (int64_t)s->rs_tail.size();
                s->rs_n_in += n[b];
                s->rs_n_out += (int64_t)conv[(size_t)b].size();
                const int64_t keep = std::min(plan->keep_from(s->rs_n_out), s->rs_n_in);
                s->rs_tail.insert(s->rs_tail.end(), samples[b], samples[b] + n[b]);
                s->rs_tail.erase(s->rs_tail.begin(), s->rs_tail.begin() + (keep - x0));
            }
            const int64_t used = j.n * c.fbank.frame_shift, len = j.n_head + j.n_tail;   // samples consumed by whole frame shifts
            std::vector<float> rem((size_t)(len - used));
            for (int64_t k = used; k < len; k++) rem[(size_t)(k - used)] = k < j.n_head ? j.head[k] : j.tail[k - j.n_head];
            s->remainder.swap(rem);
        }
    });
}
int32_t k2hip_vad_stream_is_speech(const k2hip_vad_stream_t* s) { return s ? s->st.trig : -1; }
int64_t k2hip_vad_stream_num_frames(const k2hip_vad_stream_t* s) { return s ? s->st.frames : -1; }
int32_t k2hip_vad_stream_num_segments(const k2hip_vad_stream_t* s) { return s ? (int32_t)s->segs.size() : -1; }
int32_t k2hip_vad_stream_get_segments(const k2hip_vad_stream_t* s, int64_t* start, int64_t* end, int32_t* forced, int32_t cap) {
    return guard([&] {
        NEED(s);
        if ((int64_t)s->segs.size() > cap) failf(K2HIP_ERR_CAPACITY, "stream holds %zu segments", s->segs.size());
        if (s->segs.empty()) return;
        NEED(start); NEED(end); NEED(forced);
        for (size_t i = 0; i < s->segs.size(); i++) {
            start[i] = s->segs[i].start;
            end[i] = s->segs[i].end;
            forced[i] = s->segs[i].forced;
        }
    });
}
int32_t k2hip_vad_stream_pop_segments(k2hip_vad_stream_t* s, int32_t n) {
    return guard([&] {
        NEED(s);
        K2_REQUIRE(n >= 0 && (size_t)n <= s->segs.size(), "vad_stream_pop_segments: %d of %zu segments", n, s->segs.size());
        s->segs.erase(s->segs.begin(), s->segs.begin() + n);
    });
}

int32_t k2hip_offline_recognize_long(k2hip_model_t* model, int32_t sample_rate, const float* samples, int64_t n, const k2hip_vad_config* cfg,
                                     int32_t max_batch, int64_t max_batch_frames, k2hip_long_result_t** result) {
    return guard([&] {
        NEED(model); NEED(result);
        *result = nullptr;
        K2_REQUIRE(n >= 0 && n < kResampleMaxInput, "recognize_long: %lld samples", (long long)n);
        if (n > 0) NEED(samples);
        K2_REQUIRE(max_batch > 0 && max_batch_frames > 0, "recognize_long: max_batch = %d, max_batch_frames = %lld", max_batch, (long long)max_batch_frames);
        Engine& e = model->engine;
        const Config& c = e.model().cfg();
        k2hip_vad_config use;
        if (cfg) use = *cfg;
        else vad_default_config(c.fbank.sample_rate, c.feat, c.fbank.low_freq, c.fbank.high_freq, &use);
        vad_check_config(use, c.feat);
        const ResamplePlan* plan = model_resample_plan(model, sample_rate);
        const int64_t n_own = plan ? plan->num_out(n) : n;
        if (n_own > Engine::kLongMaxSamples)
            failf(K2HIP_ERR_UNSUPPORTED, "recognize_long: %lld samples at the model's rate exceed the limit of %lld (split the recording)", (long long)n_own,
                  (long long)Engine::kLongMaxSamples);
        auto r = std::make_unique<k2hip_long_result>();
        EngineLock lk(e);
        std::vector<float> conv;
        if (plan && n_own > 0) {
            conv.resize((size_t)n_own);
            const Engine::ResampleJob job{plan, samples, n, nullptr, 0, 0, 0, n_own, conv.data()};
            e.resample_host(&job, 1);
        }
        if (n_own > 0) e.recognize_long(plan ? conv.data() : samples, n_own, use, max_batch, max_batch_frames, &r->segs);
        *result = r.release();
    });
}
int32_t k2hip_long_result_num_segments(const k2hip_long_result_t* r) { return r ? (int32_t)r->segs.size() : -1; }
int32_t k2hip_long_result_get_segment(const k2hip_long_result_t* r, int32_t i, int64_t* start, int64_t* end, int32_t* forced, int32_t* batch) {
    return guard([&] {
        NEED(r);
        K2_REQUIRE(i >= 0 && (size_t)i < r->segs.size(), "long_result_get_segment: segment %d of %zu", i, r->segs.size());
        const Engine::LongSegment& g = r->segs[(size_t)i];
        if (start) *start = g.start;
        if (end) *end = g.end;
        if (forced) *forced = g.forced;
        if (batch) *batch = g.batch;
    });
}
int32_t k2hip_long_result_get_tokens(const k2hip_long_result_t* r, int32_t i, int64_t* tokens, int32_t* timestamps, int32_t cap, int32_t* n) {
    return guard([&] {
        NEED(r); NEED(n);
        K2_REQUIRE(i >= 0 && (size_t)i < r->segs.size(), "long_result_get_tokens: segment %d of %zu", i, r->segs.size());
        const Engine::LongSegment& g = r->segs[(size_t)i];
        *n = (int32_t)g.tokens.size();
        if ((int64_t)g.tokens.size() > cap) failf(K2HIP_ERR_CAPACITY, "segment %d holds %zu tokens, capacity %d", i, g.tokens.size(), cap);
        if (g.tokens.empty()) return;
        NEED(tokens); NEED(timestamps);
        memcpy(tokens, g.tokens.data(), sizeof(int64_t) * g.tokens.size());
        memcpy(timestamps, g.timestamps.data(), sizeof(int32_t) * g.timestamps.size());
    });
}
int32_t k2hip_long_result_destroy(k2hip_long_result_t* r) {
    return guard([&] { delete r; });
}

// test hooks (include/k2hip_debug.h)
int32_t k2hip_debug_vad_check_config(const k2hip_vad_config* cfg, int32_t num_bins) {
    return guard([&] {
        NEED(cfg);
        vad_check_config(*cfg, num_bins);
    });
}
int32_t k2hip_debug_vad_default_config(int32_t sample_rate, int32_t num_bins, float low_freq, float high_freq, k2hip_vad_config* cfg) {
    return guard([&] {
        NEED(cfg);
        K2_REQUIRE(sample_rate > 0 && num_bins > 0, "vad_default_config: %d Hz, %d bins", sample_rate, num_bins);
        vad_default_config(sample_rate, num_bins, low_freq, high_freq, cfg);
    });
}
int32_t k2hip_debug_vad_pack(const int64_t* len, int32_t n, int32_t max_batch, int64_t max_batch_frames, int32_t* batch_of) {
    return guard([&] {
        K2_REQUIRE(n >= 0, "vad_pack: %d segments", n);
        if (n > 0) { NEED(len); NEED(batch_of); }
        std::vector<int32_t> b;
        vad_pack_batches(len, n, max_batch, max_batch_frames, &b);
        if (n > 0) memcpy(batch_of, b.data(), sizeof(int32_t) * (size_t)n);
    });
}
int32_t k2hip_debug_vad_ref_stream_create(int32_t num_bins, const k2hip_vad_config* cfg, k2hip_vad_stream_t** out) {
    return guard([&] {
        NEED(cfg); NEED(out);
        *out = nullptr;
        K2_REQUIRE(num_bins > 0, "vad_ref_stream_create: %d bins", num_bins);
        vad_check_config(*cfg, num_bins);
        auto s = std::make_unique<k2hip_vad_stream>();
        s->num_bins = num_bins;
        s->cfg = *cfg;
        *out = s.release();
    });
}
int32_t k2hip_debug_vad_ref_push(k2hip_vad_stream_t* s, const float* feats, int64_t n, float* tap_m, float* tap_n, uint8_t* tap_d) {
    return guard([&] {
        NEED(s);
        K2_REQUIRE(n >= 0, "vad_ref_push: %lld frames", (long long)n);
        if (n > 0) NEED(feats);
        vad_ref_push(s->cfg, s->st, feats, n, s->num_bins, &s->segs, tap_m, tap_n, tap_d);
    });
}
int32_t k2hip_debug_vad_taps(k2hip_model_t* model, int32_t b, float* m, float* n, uint8_t* d, int64_t cap, int64_t* n_frames) {
    return guard([&] {
        NEED(model); NEED(n_frames);
        EngineLock lk(model->engine);
        const Engine::VadTaps& t = model->engine.last_vad_taps();
        K2_REQUIRE(b >= 0 && (size_t)b + 1 < t.off.size(), "vad_taps: stream %d of the last call's %zu", b, t.off.empty() ? (size_t)0 : t.off.size() - 1);
        const int64_t o = t.off[(size_t)b], cnt = t.off[(size_t)b + 1] - o;
        *n_frames = cnt;
        if (cnt > cap) failf(K2HIP_ERR_CAPACITY, "vad_taps: %lld frames, capacity %lld", (long long)cnt, (long long)cap);
        if (m && cnt) memcpy(m, t.m.data() + o, sizeof(float) * (size_t)cnt);
        if (n && cnt) memcpy(n, t.n.data() + o, sizeof(float) * (size_t)cnt);
        if (d && cnt) memcpy(d, t.d.data() + o, (size_t)cnt);
    });
}
int32_t k2hip_debug_long_timing(k2hip_model_t* model, double* ms3) {
    return guard([&] {
        NEED(model); NEED(ms3);
        EngineLock lk(model->engine);
        for (int i = 0; i < 3; i++) ms3[i] = model->engine.last_long_ms()[(size_t)i];
    });
}

}  // extern "C"

// ---- neural LM rescoring (include/k2hip.h; rnn_lm_ref.h, rnn_lm_plan.h, rnn_lm.hip, rnn_lm_engine.cpp) ------------------------------
// The handle shares the immutable LM with every model it was set on: destroying it never pulls the weights from under a model.
struct k2hip_rnn_lm {
    std::shared_ptr<const RnnLm> lm;
};

extern "C" {

int32_t k2hip_rnn_lm_load(const char* path, k2hip_rnn_lm_t** out) {
    return guard([&] {
        NEED(path); NEED(out);
        *out = nullptr;
        std::shared_ptr<const RnnLm> lm(rnn_lm_load(path));
        *out = new k2hip_rnn_lm{std::move(lm)};
    });
}
int32_t k2hip_rnn_lm_destroy(k2hip_rnn_lm_t* lm) {
    return guard([&] { delete lm; });
}
int32_t k2hip_rnn_lm_vocab_size(const k2hip_rnn_lm_t* lm) { return lm ? lm->lm->V : -1; }
int32_t k2hip_rnn_lm_embedding_dim(const k2hip_rnn_lm_t* lm) { return lm ? lm->lm->E : -1; }
int32_t k2hip_rnn_lm_hidden_dim(const k2hip_rnn_lm_t* lm) { return lm ? lm->lm->H : -1; }
int32_t k2hip_rnn_lm_num_layers(const k2hip_rnn_lm_t* lm) { return lm ? lm->lm->L : -1; }
int32_t k2hip_rnn_lm_sos_id(const k2hip_rnn_lm_t* lm) { return lm ? lm->lm->sos : -1; }
int32_t k2hip_rnn_lm_eos_id(const k2hip_rnn_lm_t* lm) { return lm ? lm->lm->eos : -1; }
int32_t k2hip_rnn_lm_score_host(const k2hip_rnn_lm_t* lm, const int64_t* tokens, const int64_t* offsets, int32_t Hn, int32_t with_eos,
                                float* token_log_probs, float* totals) {
    return guard([&] {
        NEED(lm);
        K2_REQUIRE(Hn >= 0, "rnn_lm_score_host: %d hypotheses", Hn);
        if (Hn == 0) return;
        NEED(offsets); NEED(totals);
        rnn_lm_ref_score_all(*lm->lm, tokens, offsets, Hn, with_eos != 0, token_log_probs, totals);
    });
}
int32_t k2hip_set_rnn_lm(k2hip_model_t* model, const k2hip_rnn_lm_t* lm, float scale) {
    return guard([&] {
        NEED(model);
        Engine& e = model->engine;
        if (lm) {
            const int V = e.model().cfg().V;
            K2_REQUIRE(std::isfinite(scale) && scale >= 0.f, "set_rnn_lm: scale %g must be finite and >= 0", (double)scale);
            K2_REQUIRE(lm->lm->V == V, "set_rnn_lm: the LM was built for vocab_size %d, the model has %d", lm->lm->V, V);
        }
        EngineLock lk(e);
        K2_REQUIRE(e.batches_in_flight() == 0, "set_rnn_lm: %d submitted batches are in flight; wait for them first", e.batches_in_flight());
        void* dev = nullptr;
        RnnLmDev tables;
        void* fuse = nullptr;
        if (lm) dev = e.rnn_lm_upload(*lm->lm, &tables);   // (a failed upload leaves the setting as it was)
        if (lm && (model->rnn_fusion || model->rnn_stream_fusion)) {   // (a model that only rescores never pays for the fused layouts)
            try {
                fuse = e.rnn_lm_fusion_upload(*lm->lm, &tables);
            } catch (...) {
                try { e.dev_free(dev); } catch (...) {}
                throw;
            }
        }
        void *old = model->rnn_dev, *old_fuse = model->rnn_fuse_dev;
        model->rnn_dev = dev;
        model->rnn_fuse_dev = fuse;
        model->rnn_lm = lm ? lm->lm : nullptr;
        model->rnn_scale = lm ? scale : 0.f;
        model->rnn_serial++;   // (streams that carry the replaced LM's state refuse their next chunk until they are reset)
        e.set_rnn_lm(model->rnn_lm.get(), tables);
        e.set_rnn_lm_fusion(model->rnn_fusion, model->rnn_scale);
        e.set_rnn_lm_stream_fusion(model->rnn_stream_fusion);
        if (old || old_fuse) {
            e.synchronize();
            if (old) e.dev_free(old);
            if (old_fuse) e.dev_free(old_fuse);
        }
    });
}
int32_t k2hip_set_rnn_lm_fusion(k2hip_model_t* model, int32_t on) {
    return guard([&] {
        NEED(model);
        Engine& e = model->engine;
        EngineLock lk(e);
        K2_REQUIRE(e.batches_in_flight() == 0, "set_rnn_lm_fusion: %d submitted batches are in flight; wait for them first", e.batches_in_flight());
        if (on && model->rnn_lm && !model->rnn_fuse_dev) {   // the fused layouts of the attached LM, on first use
            RnnLmDev tables = e.rnn_lm_dev();
            model->rnn_fuse_dev = e.rnn_lm_fusion_upload(*model->rnn_lm, &tables);
            e.set_rnn_lm(model->rnn_lm.get(), tables);
        }
        model->rnn_fusion = on != 0;
        e.set_rnn_lm_fusion(model->rnn_fusion, model->rnn_scale);
    });
}
int32_t k2hip_set_rnn_lm_stream_fusion(k2hip_model_t* model, int32_t on) {
    return guard([&] {
        NEED(model);
        Engine& e = model->engine;
        EngineLock lk(e);
        if (on && model->rnn_lm && !model->rnn_fuse_dev) {   // the fused layouts of the attached LM, on first use
            RnnLmDev tables = e.rnn_lm_dev();
            model->rnn_fuse_dev = e.rnn_lm_fusion_upload(*model->rnn_lm, &tables);
            e.set_rnn_lm(model->rnn_lm.get(), tables);
        }
        model->rnn_stream_fusion = on != 0;
        e.set_rnn_lm_stream_fusion(model->rnn_stream_fusion);
    });
}
int32_t k2hip_debug_rnn_lm_stream_fusion_stats(k2hip_model_t* model, int64_t* chunk_calls, int64_t* live_blocks, int64_t* pool_bytes) {
    return guard([&] {
        NEED(model);
        EngineLock lk(model->engine);
        const NlmStreamPool::Stats st = model->nlm_pool ? model->nlm_pool->stats() : NlmStreamPool::Stats{};
        if (chunk_calls) *chunk_calls = beam_nlm_stream_launch_count();
        if (live_blocks) *live_blocks = st.live;
        if (pool_bytes) *pool_bytes = st.bytes;
    });
}
int32_t k2hip_rnn_lm_score(k2hip_model_t* model, const int64_t* tokens, const int64_t* offsets, int32_t Hn, int32_t with_eos,
                           float* token_log_probs, float* totals) {
    return guard([&] {
        NEED(model);
        K2_REQUIRE(Hn >= 0, "rnn_lm_score: %d hypotheses", Hn);
        EngineLock lk(model->engine);
        K2_REQUIRE(model->engine.has_rnn_lm(), "rnn_lm_score: no LM is attached to the model (k2hip_set_rnn_lm)");
        if (Hn == 0) return;
        NEED(offsets); NEED(totals);
        model->engine.rnn_lm_score_host(tokens, offsets, Hn, with_eos != 0, token_log_probs, totals);
    });
}
int32_t k2hip_offline_stream_get_alternative_lodr_score(const k2hip_offline_stream_t* s, int32_t i, float* lodr_total) {
    return guard([&] {
        NEED(s); NEED(lodr_total);
        K2_REQUIRE(i >= 0 && i < (int32_t)s->alts.size(), "alternative %d of %zu", i, s->alts.size());
        *lodr_total = s->alts[(size_t)i].lodr_score;
    });
}
int32_t k2hip_offline_stream_get_alternative_lm_score(const k2hip_offline_stream_t* s, int32_t i, float* lm_total) {
    return guard([&] {
        NEED(s); NEED(lm_total);
        K2_REQUIRE(i >= 0 && i < (int32_t)s->alts.size(), "alternative %d of %zu", i, s->alts.size());
        *lm_total = s->alts[(size_t)i].lm_score;
    });
}

// test and tuning hooks (include/k2hip_debug.h)
int32_t k2hip_debug_rnn_lm_plan(const int64_t* offsets, int32_t Hn, int32_t with_eos, int32_t H, int64_t gx_cap_floats, int32_t* order,
                                int32_t* active, int64_t* base, int32_t* block, int32_t cap_T, int32_t* T, int32_t* n_blocks) {
    return guard([&] {
        NEED(T); NEED(n_blocks);
        K2_REQUIRE(Hn >= 0 && H > 0 && cap_T >= 0, "rnn_lm_plan: %d hypotheses, hidden_dim %d", Hn, H);
        if (Hn > 0) NEED(offsets);
        for (int i = 0; i < Hn; i++)
            K2_REQUIRE(offsets[i + 1] >= offsets[i] && offsets[0] >= 0, "rnn_lm_plan: hypothesis %d: offsets decrease", i);
        const RnnLmPlan p = rnn_lm_plan(offsets, Hn, with_eos != 0, H, gx_cap_floats > 0 ? gx_cap_floats : kRnnLmGxCapFloats);
        *T = p.T;
        *n_blocks = (int32_t)p.block.size() - 1;
        if (p.T > cap_T) failf(K2HIP_ERR_CAPACITY, "rnn_lm_plan: %d positions, capacity %d", p.T, cap_T);
        if (Hn > 0) {
            NEED(order);
            memcpy(order, p.order.data(), sizeof(int32_t) * (size_t)Hn);
        }
        NEED(base); NEED(block);
        if (p.T > 0) {
            NEED(active);
            memcpy(active, p.active.data(), sizeof(int32_t) * (size_t)p.T);
        }
        memcpy(base, p.base.data(), sizeof(int64_t) * ((size_t)p.T + 1));
        memcpy(block, p.block.data(), sizeof(int32_t) * p.block.size());
    });
}
int32_t k2hip_debug_rnn_lm_stats(k2hip_model_t* model, int64_t* device_calls, int32_t* last_blocks) {
    return guard([&] {
        NEED(model);
        EngineLock lk(model->engine);
        if (device_calls) *device_calls = model->engine.rnn_lm_device_calls();
        if (last_blocks) *last_blocks = model->engine.rnn_lm_last_blocks();
    });
}
int32_t k2hip_debug_rnn_lm_fusion_stats(k2hip_model_t* model, int64_t* searches, int64_t* swept, int64_t* idle) {
    return guard([&] {
        NEED(model);
        EngineLock lk(model->engine);
        if (searches) *searches = beam_nlm_launch_count();
        model->engine.rnn_lm_fusion_work(swept, idle);
    });
}
int32_t k2hip_debug_nlm_advance_bench(k2hip_model_t* model, int32_t rows, int32_t H, int32_t iters, float* ms) {
    return guard([&] {
        NEED(model); NEED(ms);
        EngineLock lk(model->engine);
        model->engine.nlm_advance_bench(rows, H, iters, ms);
    });
}
int32_t k2hip_debug_rnn_lm_timing(k2hip_model_t* model, int32_t on, double* ms4) {
    return guard([&] {
        NEED(model);
        EngineLock lk(model->engine);
        model->engine.set_rnn_lm_timing(on != 0);
        if (ms4)
            for (int i = 0; i < 4; i++) ms4[i] = model->engine.rnn_lm_last_ms()[(size_t)i];
    });
}
int32_t k2hip_debug_rnn_lm_step_bench(k2hip_model_t* model, int32_t rows, int32_t H, int32_t iters, float* fused_ms, float* composed_ms) {
    return guard([&] {
        NEED(model);
        EngineLock lk(model->engine);
        model->engine.rnn_lm_step_bench(rows, H, iters, fused_ms, composed_ms);
    });
}

}  // extern "C"
