#include <cstring>
#include <thread>

#include "engine.h"
#include "lattice_ref.h"
#include "ctc_lattice_ref.h"
#include "kws_ref.h"
#include "ctc_kws_ref.h"
#include "ctc_prefix_bias_ref.h"
#include "ctc_prefix_ref.h"
#include "hotwords.h"
#include "ngram_lm.h"

#include <climits>
#include <cmath>

namespace k2hip {

namespace {
constexpr int kTailFrames = 19;  // PadHelper.cs:17
}

Engine::Engine(const std::string& weights, const char* overrides, int device) : device_(device) {
    // the container is parsed and validated on the host first: a missing / truncated / mismatched file is K2HIP_ERR_IO
    // whether or not a GPU is present
    tunables_init_from_env();   // (first: the model's load-time repacks read switches too)
    model_.reset(new Model(weights, overrides));
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        failf(K2HIP_ERR_NO_DEVICE, "no HIP device visible: libk2hip has no CPU fallback");
    if (device < 0 || device >= n) failf(K2HIP_ERR_NO_DEVICE, "device %d out of range (have %d)", device, n);
    K2_HIP(hipSetDevice(device));
    model_->upload(device);
    K2_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    K2_HIP(hipStreamCreateWithFlags(&stream2_, hipStreamNonBlocking));
    tunables_init_from_env();
    for (auto& sl : slots_) {
        // Streams in creation order: encoder, shared search stream, slot 0, slot 1 -- and slot 2's only at its first use (the
        // three-deep pipeline of the beam search).  HIP streams share a handful of hardware queues: with a fifth stream created
        // here the samples' H2D copy of every third batch queued behind the encoder instead of running under it (+1 ms per batch
        // from host memory), and creating the search stream AFTER slot 0's cost the same leg 1.8 ms; measured, not derived.
        if (&sl - slots_ < 2) K2_HIP(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
        K2_HIP(hipEventCreateWithFlags(&sl.enc_done, hipEventDisableTiming));
        K2_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        K2_HIP(hipEventCreateWithFlags(&sl.h2d_done, hipEventDisableTiming));
    }
    for (auto& e : ev_) K2_HIP(hipEventCreate(&e));
    K2_HIP(hipMalloc(&d_screen_counts_, 2 * sizeof(unsigned long long)));
    K2_HIP(fill_blocking(d_screen_counts_, 0, 2 * sizeof(unsigned long long)));
    // The search tables (groups = 1 decoders: the per-token conv contributions; small vocabularies: the all-contexts decoder table,
    // 0.5 GB at V = 500 -- k2hip.h "memory") are built HERE, not inside the first search call: their hipMalloc + build + stream
    // synchronisation would otherwise sit under the engine lock in the first decode or the first pipelined submit.
    if (!model_->cfg().ctc) (void)decjoin();
}

Engine::~Engine() {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (stream2_) (void)hipStreamSynchronize(stream2_);
    for (auto& sl : slots_) {
        if (sl.enc_done) (void)hipEventDestroy(sl.enc_done);
        if (sl.done) (void)hipEventDestroy(sl.done);
        if (sl.h2d_done) (void)hipEventDestroy(sl.h2d_done);
        if (sl.pin) (void)hipHostFree(sl.pin);
        if (sl.stream) { (void)hipStreamSynchronize(sl.stream); (void)hipStreamDestroy(sl.stream); }
        sl.arena.release();
    }
    if (stream2_) (void)hipStreamDestroy(stream2_);
    for (auto& kv : pe_cache_) (void)hipFree(kv.second);
    for (auto& kv : pp_cache_) (void)hipFree(kv.second);
    for (auto& kv : sinus_cache_) (void)hipFree(kv.second);
    for (auto& kv : rs_cache_) (void)hipFree(kv.second.base);
    if (online_pool_) (void)hipFree(online_pool_);
    if (d_ptab_) (void)hipFree(d_ptab_);
    if (d_dec_table_) (void)hipFree(d_dec_table_);
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : evpool_) (void)hipEventDestroy(e);
    if (d_dec_start_) (void)hipFree(d_dec_start_);
    if (d_screen_counts_) (void)hipFree(d_screen_counts_);
    if (pin_) (void)hipHostFree(pin_);
    if (pin_in_) (void)hipHostFree(pin_in_);
    if (pin_fb_) (void)hipHostFree(pin_fb_);
    arena_.release();
    if (stream_) (void)hipStreamDestroy(stream_);
}

void* Engine::pinned_in(int64_t bytes) {
    if (bytes > pin_in_cap_) {
        if (pin_in_) K2_HIP(hipHostFree(pin_in_));
        pin_in_ = nullptr;
        pin_in_cap_ = 0;
        K2_HIP(hipHostMalloc(&pin_in_, (size_t)(bytes + bytes / 4), hipHostMallocDefault));
        pin_in_cap_ = bytes + bytes / 4;
    }
    return pin_in_;
}

void* Engine::pinned_fb(int64_t bytes) {
    if (bytes > pin_fb_cap_) {
        K2_REQUIRE(!fb_pending_.active, "internal: the fbank staging buffer grows under a deferred gather");
        if (pin_fb_) K2_HIP(hipHostFree(pin_fb_));
        pin_fb_ = nullptr;
        pin_fb_cap_ = 0;
        K2_HIP(hipHostMalloc(&pin_fb_, (size_t)(bytes + bytes / 4), hipHostMallocDefault));
        pin_fb_cap_ = bytes + bytes / 4;
    }
    return pin_fb_;
}

void* Engine::pinned(int64_t bytes) {
    if (bytes > pin_cap_) {
        if (pin_) K2_HIP(hipHostFree(pin_));
        pin_ = nullptr;
        pin_cap_ = 0;
        K2_HIP(hipHostMalloc(&pin_, (size_t)bytes, hipHostMallocDefault));
        pin_cap_ = bytes;
    }
    return pin_;
}

Ctx Engine::make_ctx(bool dry) {
    Ctx c;
    c.stream = stream_;
    c.arena = cur_arena_;
    c.dry = dry;
    c.instrument = instrument_ && !dry;
    c.stats = &stats_;
    c.evpool = &evpool_;
    c.evused = &evused_;
    c.gemm_log = &gemm_log_;
    c.greedy_rec = &last_greedy_;
    c.one_part = one_part_left_ > 0;
    return c;
}

int Engine::encoder_out_frames(int T) const {
    if (model_->cfg().conformer) return conformer_out_frames(T);
    if (model_->cfg().lstm) return lstm_out_frames(T);
    int T50 = (T - 7) / 2;
    return T50 <= 0 ? 0 : (T50 + 1) / 2;
}
int64_t Engine::fbank_num_frames(int64_t n) const {
    const FbankOpts& f = model_->cfg().fbank;
    if (n < f.frame_len) return 0;
    return 1 + (n - f.frame_len) / f.frame_shift;
}

// CompactRelPositionalEncoding (icefall zipformer.py): row n <-> relative offset n-(T-1)
const float* Engine::pos_emb(int T) {
    auto it = pe_cache_.find(T);
    if (it != pe_cache_.end()) return it->second;
    const int pd = model_->cfg().pos_dim, n2 = 2 * T - 1;
    std::vector<float> pe((size_t)n2 * pd);
    const float cl = sqrtf((float)pd), ls = (float)pd / (2.0f * (float)M_PI), logcl = logf(cl);
    for (int n = 0; n < n2; n++) {
        float x = (float)(n - (T - 1));
        float sg = (float)((x > 0.f) - (x < 0.f));
        float xa = atanf(cl * sg * (logf(fabsf(x) + cl) - logcl) / ls);
        for (int k = 0; k < pd / 2; k++) {
            pe[(size_t)n * pd + 2 * k] = cosf(xa * (float)(k + 1));
            pe[(size_t)n * pd + 2 * k + 1] = sinf(xa * (float)(k + 1));
        }
        pe[(size_t)n * pd + pd - 1] = 1.0f;
    }
    float* d = nullptr;
    K2_HIP(hipMalloc(&d, pe.size() * sizeof(float)));
    K2_HIP(copy_blocking(d, pe.data(), pe.size() * sizeof(float), hipMemcpyHostToDevice));
    pe_cache_[T] = d;
    return d;
}

DecJoinW Engine::decjoin() {
    std::lock_guard<std::mutex> lk(cache_mu_);
    const Config& c = model_->cfg();
    DecJoinW w;
    w.emb = model_->w("decoder.embedding.weight");
    w.cpg = c.conv_cpg;
    K2_REQUIRE(w.cpg <= 4 || w.cpg == c.DD, "decoder conv with %d channels per group: only <= 4 or groups = 1 are built", w.cpg);
    w.conv = model_->w(w.cpg > 4 ? "decoder.conv.weight#kn" : "decoder.conv.weight");
    w.dproj_kn = model_->w("joiner.decoder_proj.weight#kn");
    w.dproj_b = model_->w("joiner.decoder_proj.bias");
    w.out_kn = model_->w("joiner.output_linear.weight#kn");
    w.out_b = model_->w("joiner.output_linear.bias");
    w.V = c.V; w.Vp = c.Vp; w.DD = c.DD; w.J = c.J; w.ctx = c.ctx;
    if (model_->has("joiner.output_linear.weight#h16") && tunables().screen_min_v > 0) {
        w.out_h16 = model_->w("joiner.output_linear.weight#h16");
        w.out_eps = model_->w("joiner.output_linear.weight#eps");
        w.out_vj = model_->w("joiner.output_linear.weight");
    }
    if (w.cpg > 4) {
        if (!d_ptab_) {  // one-off: P[tap] = emb . conv_tap^T on the MFMA GEMM
            K2_HIP(hipMalloc(&d_ptab_, sizeof(float) * 2 * (size_t)c.V * c.DD));
            Ctx t;
            t.stream = stream_;
            for (int tap = 0; tap < 2; tap++)
                linear(t, w.emb, c.DD, model_->w("decoder.conv.weight#tap" + std::to_string(tap)), nullptr,
                       d_ptab_ + (size_t)tap * c.V * c.DD, c.DD, c.V, c.DD, c.DD);
            K2_HIP(hipStreamSynchronize(stream_));
        }
        w.ptab = d_ptab_;
    }
    // Every context's decoder output, when the vocabulary is small enough (V = 500: 250 500 rows x 2 KB = 0.5 GB of the 288):
    // an emission's decoder update in the search loops is then one row read instead of a 1 MB GEMV through one CU.
    const size_t table_bytes = sizeof(float) * ((size_t)c.V + 1) * c.V * c.J;
    if (!dec_table_tried_ && tunables().decoder_table_mb > 0 && table_bytes <= (size_t)tunables().decoder_table_mb << 20 &&
        c.J % 4 == 0 && c.DD % 4 == 0) {
        dec_table_tried_ = true;
        if (hipMalloc(&d_dec_table_, table_bytes) == hipSuccess) {
            Ctx t;
            t.stream = stream_;
            decoder_table(t, w, d_dec_table_);
            K2_HIP(hipStreamSynchronize(stream_));
        } else {
            (void)hipGetLastError();   // no room: the loops run the decoder themselves
            d_dec_table_ = nullptr;
        }
    }
    w.dec_table = d_dec_table_;
    return w;
}

void Engine::decoder_table_check(int n_samples, unsigned seed, long long* rows, long long* mismatched) {
    const DecJoinW w = decjoin();
    *rows = 0;
    *mismatched = 0;
    if (!w.dec_table) return;
    const long long V = w.V, n_ctx = (V + 1) * V;
    *rows = n_ctx;
    std::vector<long long> y;
    auto add = [&](long long y0, long long y1) { y.push_back(y0); y.push_back(y1); };
    add(-1, K2HIP_BLANK_ID);
    add(K2HIP_BLANK_ID, K2HIP_BLANK_ID);
    add(-1, V - 1);
    add(V - 1, V - 1);
    unsigned long long st = seed * 6364136223846793005ull + 1442695040888963407ull;
    for (int i = 0; i < n_samples; i++) {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        const long long cx = (long long)((st >> 20) % (unsigned long long)n_ctx);
        add(cx / V - 1, cx % V);
    }
    const int N = (int)(y.size() / 2);
    long long* d_y = nullptr;
    float* d_out = nullptr;
    K2_HIP(hipMalloc(&d_y, sizeof(long long) * y.size()));
    K2_HIP(hipMalloc(&d_out, sizeof(float) * (size_t)N * w.J));
    std::vector<float> got((size_t)N * w.J), want(w.J);
    try {
        K2_HIP(hipMemcpyAsync(d_y, y.data(), sizeof(long long) * y.size(), hipMemcpyHostToDevice, stream_));
        Ctx t;
        t.stream = stream_;
        decoder_rows_wide(t, w, d_y, N, d_out);
        K2_HIP(hipMemcpyAsync(got.data(), d_out, sizeof(float) * got.size(), hipMemcpyDeviceToHost, stream_));
        K2_HIP(hipStreamSynchronize(stream_));
        for (int n = 0; n < N; n++) {
            const long long row = (y[2 * n] + 1) * V + y[2 * n + 1];
            K2_HIP(copy_blocking(want.data(), w.dec_table + row * w.J, sizeof(float) * w.J, hipMemcpyDeviceToHost));
            for (int k = 0; k < w.J; k++) *mismatched += memcmp(&want[k], &got[(size_t)n * w.J + k], sizeof(float)) != 0;
        }
    } catch (...) {
        (void)hipFree(d_y);
        (void)hipFree(d_out);
        throw;
    }
    (void)hipFree(d_y);
    (void)hipFree(d_out);
}

// ---------------------------------------------------------------------------
// Conv2dSubsampling (encoder_embed), NHWC.  x: [B,T,80] -> [B,T50,D0]
// ---------------------------------------------------------------------------
float* Engine::encoder_embed(const Ctx& c, const float* x, int B, int T, int* T50) {
    const Model& m = *model_;
    const int F0 = 80, T1 = T - 2, T2 = (T1 - 3) / 2 + 1, F2 = (F0 - 3) / 2 + 1, T3 = T2 - 2, F3 = (F2 - 3) / 2 + 1;
    K2_REQUIRE(T3 > 0, "encoder: %d input frames are too few (need >= 9)", T);
    Arena& ar = *c.arena;
    const int D0 = m.cfg().dim[0];
    float* out = ar.take<float>((int64_t)B * T3 * D0);
    int64_t mark = ar.mark();
    float* a1 = ar.take<float>((int64_t)B * T1 * F0 * 8);
    conv0_swoosh(c, x, m.w("encoder_embed.conv.0.weight"), m.w("encoder_embed.conv.0.bias"), a1, B, T, F0);
    c.add_flops(0, 2.0 * B * T1 * (double)F0 * 8 * 9, 0);
    float* a2 = ar.take<float>((int64_t)B * T2 * F2 * 32);
    {
        GemmArgs g;
        g.A = a1; g.W = m.w("encoder_embed.conv.4.weight#ohwi"); g.ldw = 72; g.bias = m.w("encoder_embed.conv.4.bias");
        g.C = a2; g.ldc = 32; g.M = B * T2 * F2; g.N = 32; g.K = 72; g.act = ACT_SWOOSH_R;
        g.cv_Fout = F2; g.cv_Tout = T2; g.cv_Tin = T1; g.cv_Fin = F0; g.cv_C = 8; g.cv_st = 2; g.cv_sf = 2;
        g.seg_len = 24; g.seg_stride = F0 * 8;
        gemm(c, g);
    }
    float* a3 = ar.take<float>((int64_t)B * T3 * F3 * 128);
    {
        GemmArgs g;
        g.A = a2; g.W = m.w("encoder_embed.conv.7.weight#ohwi"); g.ldw = 288; g.bias = m.w("encoder_embed.conv.7.bias");
        g.C = a3; g.ldc = 128; g.M = B * T3 * F3; g.N = 128; g.K = 288; g.act = ACT_SWOOSH_R;
        g.cv_Fout = F3; g.cv_Tout = T3; g.cv_Tin = T2; g.cv_Fin = F2; g.cv_C = 32; g.cv_st = 1; g.cv_sf = 2;
        g.seg_len = 96; g.seg_stride = F2 * 32;
        gemm(c, g);
    }
    // ConvNeXt: a3 += pw2(SwooshL(pw1(dw7x7(a3))))
    const int npix = B * T3 * F3;
    float* dw = ar.take<float>((int64_t)npix * 128);
    dwconv7x7(c, a3, m.w("encoder_embed.convnext.depthwise_conv.weight#kc"), m.w("encoder_embed.convnext.depthwise_conv.bias"),
              dw, B, T3, T3, 3, F3, 128);
    float* hid = ar.take<float>((int64_t)npix * 384);
    linear(c, dw, 128, m.w("encoder_embed.convnext.pointwise_conv1.weight"), m.w("encoder_embed.convnext.pointwise_conv1.bias"),
           hid, 384, npix, 128, 384, ACT_SWOOSH_L);
    linear(c, hid, 384, m.w("encoder_embed.convnext.pointwise_conv2.weight"), m.w("encoder_embed.convnext.pointwise_conv2.bias"),
           a3, 128, npix, 384, 128, ACT_NONE, a3, 128);
    // (b,t,f,c) flatten == [B*T3, F3*128] with the repacked out.weight
    float* lin = ar.take<float>((int64_t)B * T3 * D0);
    linear(c, a3, F3 * 128, m.w("encoder_embed.out.weight#fc"), m.w("encoder_embed.out.bias"), lin, D0, B * T3, F3 * 128, D0);
    biasnorm(c, lin, m.w("encoder_embed.out_norm.bias"), m.w("encoder_embed.out_norm.log_scale"), out, B * T3, D0);
    ar.rewind(mark);
    *T50 = T3;
    return out;
}

const float* Engine::pos_proj_cached(const Ctx& c, int layer, const float* pe, int pe_dim, const float* W, int rows, int ncols) {
    if (c.dry) return nullptr;
    std::lock_guard<std::mutex> lk(cache_mu_);
    const auto key = std::make_pair(layer, rows);
    auto it = pp_cache_.find(key);
    if (it != pp_cache_.end()) return it->second;
    const size_t bytes = sizeof(float) * (size_t)rows * ncols;
    if (pp_cache_bytes_ + bytes > ((size_t)1 << 30)) {  // many distinct utterance lengths: start over (stream-ordered frees)
        synchronize();
        for (auto& kv : pp_cache_) (void)hipFree(kv.second);
        pp_cache_.clear();
        pp_cache_bytes_ = 0;
    }
    float* pp = nullptr;
    K2_HIP(hipMalloc(&pp, bytes));
    Ctx plain = c;  // not one of the call's logged / timed GEMMs
    plain.instrument = false;
    plain.gemm_log = nullptr;
    linear(plain, pe, pe_dim, W, nullptr, pp, ncols, rows, pe_dim, ncols);
    K2_HIP(hipStreamSynchronize(c.stream));  // other HIP streams of this engine may read it next
    pp_cache_[key] = pp;
    pp_cache_bytes_ += bytes;
    return pp;
}

// ---------------------------------------------------------------------------
// Zipformer2EncoderLayer.forward / .streaming_forward (inference), in place on x [B*T, D]; gl = global layer index.
// site == null: T frames of whole utterances.  Otherwise the streams' chunk of T frames behind cf.left[si] frames of left context: the
// attention weights run over the key ring, NonlinAttention and the self-attention modules over their value rings, the depthwise
// convolution is the chunk-causal one over the conv cache (slot layout: lay_, indexed by gl).  The launch skeleton is the same.
// ---------------------------------------------------------------------------
void Engine::encoder_layer(const Ctx& c, int si, int li, int gl, float* x, const float* pe, int B, int T, const StreamSite* site,
                           const LayerTail* tail) {
    const Model& m = *model_;
    const Config& cf = m.cfg();
    const int D = cf.dim[si], F = cf.ff[si], H = cf.heads[si], vh = cf.vhd[si], K = cf.kern[si], qh = cf.qhd[si], ph = cf.phd[si];
    // the keys are the T frames, behind L frames of left context when streaming; KLp = their count rounded up to 4 (a row of aw)
    const int L = site ? cf.left[si] : 0, M = B * T, KL = L + T, KLp = (KL + 3) & ~3, inproj = (2 * qh + ph) * H, Hc = 3 * D / 4, HV = H * vh;
    char p[96];
    snprintf(p, sizeof p, "encoder.encoders.%d.layers.%d.", si, li);
    auto w = [&](const char* suffix) { return m.w(std::string(p) + suffix); };
    auto wk = [&](const char* fmt, int k) {   // a weight of the k-th module of its kind: wk("self_attn%d.in_proj.weight", 2)
        char name[96];
        snprintf(name, sizeof name, fmt, k);
        return w(name);
    };
    Arena& ar = *c.arena;
    int64_t mark = ar.mark();
    const long long SS = lay_.floats_per_stream;
    auto ring = [&](long long off) {   // (streaming) a ring of the site's streams in the state pool
        RingRef r;
        r.pool = online_pool_; r.slot_stride = SS; r.off = off; r.slots = site->d_slots; r.chunks = site->d_chunks;
        return r;
    };

    // [ff1.in_proj | attention-weights in_proj] of the layer input in one GEMM (model.cpp stacks the two weight matrices);
    // the attention weights are shared by nonlin_attention / self_attn1 / self_attn2
    const int F1 = F * 3 / 4, ldcat = F1 + inproj;
    float* cat = ar.take<float>((int64_t)M * ldcat);
    {
        GemmArgs g;
        g.A = x; g.lda = D; g.W = w("#ff1_attn_in.weight"); g.ldw = D; g.bias = w("#ff1_attn_in.bias");
        g.C = cat; g.ldc = ldcat; g.M = M; g.N = ldcat; g.K = D; g.act = ACT_SWOOSH_L; g.act_cols = F1;
        gemm(c, g);
    }
    const float* qkp = cat + F1;
    // the layer's positional projection does not depend on the audio: cached per (layer, rows), streaming tables under 1000 + gl
    const float* pp = pos_proj_cached(c, site ? 1000 + gl : gl, pe, cf.pos_dim, w("self_attn_weights.linear_pos.weight"), 2 * T - 1 + L, ph * H);
    float* aw = ar.take<float>((int64_t)H * B * T * KLp);  // (streaming: columns in ring order)
    if (site) attn_stream_ring(c, qkp, ldcat, ring(lay_.key[gl]), pp, site->d_plen, aw, B, T, L, KLp, H, cf.ds[si], cf.left[0] * cf.ds[0]);
    else attn_scores_softmax(c, qkp, ldcat, pp, aw, B, T, KLp, H);

    float* src = ar.take<float>((int64_t)M * D);
    // the streaming self-attention modules with their value projection inside (attn_proj_av_out_ring) read one buffer and write the other
    const bool vproj_fused = site && !tunables().no_fused_vproj && T >= tunables().fused_vproj_min_t && D % 32 == 0 && vh <= 16 && HV % 4 == 0 && HV <= 128;
    float* src_alt = vproj_fused ? ar.take<float>((int64_t)M * D) : nullptr;
    float* hid = ar.take<float>((int64_t)M * std::max({F * 5 / 4, 3 * Hc, 2 * D}));
    float* tmp = site ? nullptr : ar.take<float>((int64_t)M * std::max(D, Hc));
    float* tmp2 = ar.take<float>((int64_t)M * std::max(D, Hc));

    auto feed_forward = [&](int k, int Fk, const float* in, float* out) {
        linear(c, in, D, wk("feed_forward%d.in_proj.weight", k), wk("feed_forward%d.in_proj.bias", k), hid, Fk, M, D, Fk, ACT_SWOOSH_L);
        linear(c, hid, Fk, wk("feed_forward%d.out_proj.weight", k), wk("feed_forward%d.out_proj.bias", k), out, D, M, Fk, D, ACT_NONE, in, D);
    };
    auto nonlin_attention = [&]() {   // src += NonlinAttention(src, aw[0])
        if (site) {
            linear(c, src, D, w("nonlin_attention.in_proj.weight"), w("nonlin_attention.in_proj.bias"), hid, 3 * Hc, M, D, 3 * Hc);
            // x * tanh(s) into the ring rows of this chunk and ctx = (aw_head0 . ring) * y in one per-stream launch
            nonlin_av_out_ring(c, aw, ring(lay_.nonlin[gl]), hid, 3 * Hc, nullptr, nullptr, tmp2, B, T, KL, KLp, Hc, D);
        } else {
            GemmArgs g;
            g.A = aw; g.lda = KLp; g.sA0 = (long long)T * KLp;
            g.w_kn = 1;
            g.C = tmp2; g.ldc = Hc; g.sC0 = (long long)T * Hc;
            g.M = T; g.N = Hc; g.K = T; g.nb0 = B; g.nb1 = 1;
            if (M >= 256 && Hc % 16 == 0 && !tunables().no_glu_epilogue) {
                // in_proj with x * tanh(s) in its epilogue (weights interleaved at load): hid = [M, 2 Hc] = (gated | y)
                GemmArgs p;
                p.A = src; p.lda = D; p.W = w("nonlin_attention.in_proj.weight#glu"); p.ldw = D; p.bias = w("nonlin_attention.in_proj.bias#glu");
                p.C = hid; p.ldc = 2 * Hc; p.M = M; p.N = 3 * Hc; p.K = D; p.glu = 2; p.glu_cols = 2 * Hc;
                gemm(c, p);
                g.W = hid; g.ldw = 2 * Hc; g.sW0 = (long long)T * 2 * Hc;
                g.mul = hid + Hc; g.ldm = 2 * Hc; g.sM0 = (long long)T * 2 * Hc;  // x * y (the third chunk of in_proj) in the epilogue
            } else {
                linear(c, src, D, w("nonlin_attention.in_proj.weight"), w("nonlin_attention.in_proj.bias"), hid, 3 * Hc, M, D, 3 * Hc);
                tanh_gate(c, hid, tmp, M, Hc);
                g.W = tmp; g.ldw = Hc; g.sW0 = (long long)T * Hc;
                g.mul = hid + 2 * Hc; g.ldm = 3 * Hc; g.sM0 = (long long)T * 3 * Hc;  // x * y (the third chunk of in_proj) in the epilogue
            }
            gemm(c, g);
        }
        linear(c, tmp2, Hc, w("nonlin_attention.out_proj.weight"), w("nonlin_attention.out_proj.bias"), src, D, M, Hc, D, ACT_NONE, src, D);
    };
    auto self_attn = [&](int k) {
        const float *wi = wk("self_attn%d.in_proj.weight", k), *bi = wk("self_attn%d.in_proj.bias", k);
        const float *wo = wk("self_attn%d.out_proj.weight", k), *bo = wk("self_attn%d.out_proj.bias", k);
        if (vproj_fused) {   // one launch: value projection of the chunk's rows, ring update, attention apply, out_proj, residual
            attn_proj_av_out_ring(c, aw, ring(k == 1 ? lay_.val1[gl] : lay_.val2[gl]), src, wi, bi, wo, bo, src_alt, B, T, KL, KLp, H, vh, D);
            std::swap(src, src_alt);
            return;
        }
        linear(c, src, D, wi, bi, hid, HV, M, D, HV);
        if (site) {   // fused: chunk rows into the value ring, attention apply over the ring, out_proj, residual
            attn_av_out_ring(c, aw, ring(k == 1 ? lay_.val1[gl] : lay_.val2[gl]), hid, wo, bo, src, B, T, KL, KLp, H, vh, D);
            return;
        }
        if (attn_av_out(c, aw, hid, wo, bo, src, B, T, T, KLp, H, vh, D)) return;  // fused attention-apply + out_proj + residual
        GemmArgs g;  // tmp[b, :, h*vh : (h+1)*vh] = aw[h][b] . hid[b, :, h*vh : ...]
        g.A = aw; g.lda = KLp; g.sA0 = (long long)T * KLp; g.sA1 = (long long)B * T * KLp;
        g.W = hid; g.w_kn = 1; g.ldw = HV; g.sW0 = (long long)T * HV; g.sW1 = vh;
        g.C = tmp; g.ldc = HV; g.sC0 = (long long)T * HV; g.sC1 = vh;
        g.M = T; g.N = vh; g.K = T; g.nb0 = B; g.nb1 = H;
        gemm(c, g);
        linear(c, tmp, HV, wo, bo, src, D, M, HV, D, ACT_NONE, src, D);
    };
    auto conv_module = [&](int k) {   // src += out_proj(SwooshR(depthwise_conv(GLU(in_proj(src)))))
        if (site) {
            const long long cache_off = k == 1 ? lay_.conv1[gl] : lay_.conv2[gl];
            const float *wc = wk("conv_module%d.depthwise_conv.causal_conv.weight", k), *bc = wk("conv_module%d.depthwise_conv.causal_conv.bias", k);
            const float *ww = wk("conv_module%d.depthwise_conv.chunkwise_conv.weight", k), *bw = wk("conv_module%d.depthwise_conv.chunkwise_conv.bias", k);
            const float* sc = wk("conv_module%d.depthwise_conv.chunkwise_conv_scale", k);
            // in_proj + GLU + chunk-causal depthwise conv + SwooshR in ONE launch where the shape has the fused form (round 5): the T rows
            // of a stream and a 16-channel (value | gate) block sit in one tile of the in_proj GEMM, so its epilogue has everything the
            // convolution needs (conv_module 3 -> 2 launches, 32 per tick; K2HIP_NO_FUSED_CONV keeps the two launches for the cross-check)
            bool fused = false;
            if (!tunables().no_fused_conv)
                fused = gemm_glu_causal_conv(c, src, wk("conv_module%d.in_proj.weight#glu", k), wk("conv_module%d.in_proj.bias#glu", k), online_pool_, SS,
                                             cache_off, site->d_slots, wc, bc, ww, bw, sc, tmp2, B, T, D, K);
            if (!fused) {
                linear(c, src, D, wk("conv_module%d.in_proj.weight", k), wk("conv_module%d.in_proj.bias", k), hid, 2 * D, M, D, 2 * D);
                glu_causal_conv(c, hid, online_pool_, SS, cache_off, site->d_slots, wc, bc, ww, bw, sc, tmp2, B, T, D, K);
            }
        } else {
            const float *wd = wk("conv_module%d.depthwise_conv.weight#kd", k), *bd = wk("conv_module%d.depthwise_conv.bias", k);
            // in_proj + GLU + depthwise conv + SwooshR in ONE launch where all T rows of a stream fit the M tile of the in_proj GEMM (the
            // low-rate stacks: T = 127 in a 128-row tile, 64 in a 64-row one): the tile that has just finished the GLU holds every frame
            // the convolution of its channels needs, and hid is never written (conv_module 3 -> 2 launches; bit-identical to the two
            // launches, which K2HIP_NO_FUSED_CONV keeps for the cross-check)
            const bool fused = gemm_glu_dwconv1d(c, src, wk("conv_module%d.in_proj.weight#glu", k), wk("conv_module%d.in_proj.bias#glu", k), wd, bd, tmp2, B, T, D, K);
            if (fused) {
                // tmp2 holds SwooshR(depthwise_conv(GLU(in_proj(src))))
            } else if (M >= 256 && !tunables().no_glu_epilogue) {
                // in_proj with the GLU in its epilogue (weights interleaved at load): hid is [M, D], not [M, 2D]
                GemmArgs g;
                g.A = src; g.lda = D; g.W = wk("conv_module%d.in_proj.weight#glu", k); g.ldw = D; g.bias = wk("conv_module%d.in_proj.bias#glu", k);
                g.C = hid; g.ldc = D; g.M = M; g.N = 2 * D; g.K = D; g.glu = 1;
                gemm(c, g);
                dwconv1d_swoosh(c, hid, wd, bd, tmp2, B, T, D, K);
            } else {
                linear(c, src, D, wk("conv_module%d.in_proj.weight", k), wk("conv_module%d.in_proj.bias", k), hid, 2 * D, M, D, 2 * D);
                glu_dwconv1d_swoosh(c, hid, wd, bd, tmp2, B, T, D, K);
            }
        }
        linear(c, tmp2, D, wk("conv_module%d.out_proj.weight", k), wk("conv_module%d.out_proj.bias", k), src, D, M, D, D, ACT_NONE, src, D);
    };

    // src = x + ff1(x): the hidden activations are the first F1 columns of `cat`
    linear(c, cat, ldcat, w("feed_forward1.out_proj.weight"), w("feed_forward1.out_proj.bias"), src, D, M, F1, D, ACT_NONE, x, D);
    nonlin_attention();
    self_attn(1);
    conv_module(1);
    {   // src = bypass_mid(x, src + ff2(src)): the bypass mix runs in the out_proj GEMM's epilogue
        linear(c, src, D, w("feed_forward2.in_proj.weight"), w("feed_forward2.in_proj.bias"), hid, F, M, D, F, ACT_SWOOSH_L);
        GemmArgs g;
        g.A = hid; g.lda = F; g.W = w("feed_forward2.out_proj.weight"); g.ldw = F; g.bias = w("feed_forward2.out_proj.bias");
        g.C = src; g.ldc = D; g.M = M; g.N = D; g.K = F; g.res = src; g.ldr = D;
        g.byp_orig = x; g.ld_orig = D; g.byp_scale = w("bypass_mid.bypass_scale");
        gemm(c, g);
    }
    self_attn(2);
    conv_module(2);
    feed_forward(3, F * 5 / 4, src, src);
    if (tail && tail->bias2)   // the stack's last layer in front of a downsampled stack: that stack's downsample in the same launch
        biasnorm_bypass_downsample(c, src, x, w("norm.bias"), w("norm.log_scale"), w("bypass.bypass_scale"), x, tail->bias2, tail->xd2, B, T, D,
                                   tail->ds2, tail->D2);
    else
        biasnorm_bypass(c, src, x, w("norm.bias"), w("norm.log_scale"), w("bypass.bypass_scale"), x, M, D);
    ar.rewind(mark);
}

// which stack output supplies which columns of the full-width row (Zipformer2._get_full_dim_output): the last stack's output, then,
// walking back, every stack that is wider than what is covered so far contributes its extra columns
static FullDimSegs full_dim_segments(const Config& cf, float* const* outputs) {
    FullDimSegs s;
    int cur = cf.dim[cf.ns - 1];
    s.src[0] = outputs[cf.ns - 1]; s.ld[0] = cur; s.col1[0] = cur; s.n = 1;
    for (int i = cf.ns - 2; i >= 0; i--) {
        const int d = cf.dim[i];
        if (d > cur) {
            K2_REQUIRE(s.n < 8, "too many stack widths");
            s.src[s.n] = outputs[i]; s.ld[s.n] = d; s.col1[s.n] = d; s.n++;
            cur = d;
        }
    }
    return s;
}

// Zipformer2.forward / .streaming_forward: the stacks over x0 [B*T50, dim[0]], whole utterances (site == null) or the site's chunk.
// Returns false with *segs = the pieces of the full-width output [B*T50, Dmax], which the caller's downsample_full gathers itself (no
// concatenated tensor); true when the walk ended in an offline tap (1 + i: the output of stack i; 100: the concatenated tensor) -- then
// *tap_ptr / *tap_dim name it and *segs is not set.  Streaming passes tap = -1.
bool Engine::encoder_stacks(const Ctx& c, float* x0, int B, int T50, const StreamSite* site, int tap, float** tap_ptr, int* tap_dim, FullDimSegs* segs) {
    const Model& m = *model_;
    const Config& cf = m.cfg();
    Arena& ar = *c.arena;
    const int M = B * T50;
    float* outputs[kMaxStacks] = {nullptr};
    float* x = x0;
    int Dcur = cf.dim[0], gl = 0;
    float *pre_y = nullptr, *pre_xd = nullptr;
    FullDimSegs lz;   // (only its lz_* fields are used)
    for (int si = 0; si < cf.ns; si++) {
        const int D = cf.dim[si], ds = cf.ds[si], nl = cf.nlayer[si];
        // the stack's input is the previous output zero-extended / truncated to D channels (convert_channels): a stack that runs at
        // the input rate works in place on a converted copy (or on x itself when the width does not change); a downsampled stack
        // never materialises it -- its downsample and its out_combiner read x at its own width
        const int Din = Dcur;
        Dcur = D;
        const int Td = (T50 + ds - 1) / ds;   // the stack's own frames
        const float* pe = c.dry ? nullptr : site ? pos_emb_stream(Td, cf.left[si]) : pos_emb(Td);
        if (ds == 1) {
            float* xi = x;
            if (D != Din) {
                xi = ar.take<float>((int64_t)M * D);
                convert_channels(c, x, xi, M, Din, D);
            }
            // in front of a downsampled stack the last layer's BiasNorm launch forms that stack's input as well (LayerTail)
            LayerTail tail;
            if (si + 1 < cf.ns && cf.ds[si + 1] > 1 && nl > 0) {
                tail.D2 = cf.dim[si + 1]; tail.ds2 = cf.ds[si + 1];
                pre_y = ar.take<float>((int64_t)M * tail.D2);
                pre_xd = ar.take<float>((int64_t)B * ((T50 + tail.ds2 - 1) / tail.ds2) * tail.D2);
                tail.xd2 = pre_xd;
                tail.bias2 = m.wf("encoder.encoders.%d.downsample.bias", si + 1);
            }
            for (int li = 0; li < nl; li++, gl++) encoder_layer(c, si, li, gl, xi, pe, B, T50, site, li == nl - 1 ? &tail : nullptr);
            x = xi;
        } else {
            // Round 5: where the NEXT stack is downsampled too, this stack's out_combiner and that stack's SimpleDownsample are one
            // launch (upsample_combine_downsample): its two outputs -- the next stack's `y` is not one of them, only reserved here -- are
            // taken in front of this stack's mark, so that they outlive the rewind.
            float* y = pre_y ? pre_y : ar.take<float>((int64_t)M * D);
            float* xd_ready = pre_xd;   // this stack's downsampled input, if the previous stack's combiner produced it
            pre_y = pre_xd = nullptr;
            const bool fuse_next = si + 1 < cf.ns && cf.ds[si + 1] > 1;
            const int D2 = fuse_next ? cf.dim[si + 1] : 0, ds2 = fuse_next ? cf.ds[si + 1] : 1;
            if (fuse_next) {
                pre_y = ar.take<float>((int64_t)M * D2);
                pre_xd = ar.take<float>((int64_t)B * ((T50 + ds2 - 1) / ds2) * D2);
            }
            int64_t mark = ar.mark();
            float* xd = xd_ready ? xd_ready : ar.take<float>((int64_t)B * Td * D);
            if (!xd_ready) downsample(c, x, m.wf("encoder.encoders.%d.downsample.bias", si), xd, B, T50, D, ds, Din);
            for (int li = 0; li < nl; li++, gl++) encoder_layer(c, si, li, gl, xd, pe, B, Td, site);
            // the LAST stack's out_combiner runs inside the final downsample (FullDimSegs::lz_*): its output tensor is never written,
            // unless a tap asks for it
            const bool lazy = si == cf.ns - 1 && tap != 1 + si && tap != 100;
            if (fuse_next)
                upsample_combine_downsample(c, x, xd, m.wf("encoder.encoders.%d.out_combiner.bypass_scale", si), y,
                                            m.wf("encoder.encoders.%d.downsample.bias", si + 1), pre_xd, B, T50, Td, D, ds, Din, D2, ds2);
            else if (lazy) {
                lz.lz_orig = c.dry ? nullptr : x; lz.lz_xd = xd; lz.lz_scale = c.dry ? nullptr : m.wf("encoder.encoders.%d.out_combiner.bypass_scale", si);
                lz.lz_Td = Td; lz.lz_ds = ds; lz.lz_Do = Din;
            } else
                upsample_combine(c, x, xd, m.wf("encoder.encoders.%d.out_combiner.bypass_scale", si), y, B, T50, Td, D, ds, Din);
            if (!lazy) ar.rewind(mark);   // (lazy: xd is read by the final downsample -- it stays allocated)
            x = y;
        }
        outputs[si] = x;
        if (tap == 1 + si) {
            *tap_ptr = x;
            *tap_dim = D;
            return true;
        }
    }
    if (tap == 100) {   // _get_full_dim_output as a tensor
        float* full = ar.take<float>((int64_t)M * cf.dmax);
        const FullDimSegs s = full_dim_segments(cf, outputs);
        for (int i = 0, col0 = 0; i < s.n; i++) {
            copy_cols(c, s.src[i], s.ld[i], col0, full, cf.dmax, col0, M, s.col1[i] - col0);
            col0 = s.col1[i];
        }
        *tap_ptr = full;
        *tap_dim = cf.dmax;
        return true;
    }
    *segs = full_dim_segments(cf, outputs);
    segs->lz_orig = lz.lz_orig; segs->lz_xd = lz.lz_xd; segs->lz_scale = lz.lz_scale;
    segs->lz_Td = lz.lz_Td; segs->lz_ds = lz.lz_ds; segs->lz_Do = lz.lz_Do;
    return false;
}

// encoder.downsample_output over the stacks' full-width output, then the model's head: joiner.encoder_proj, or a CTC model's
// Linear(Dmax -> V) + log_softmax (its "log_probs" output).  Returns [B * T', enc_dim] in enc_out, or (null) taken here, last.
float* Engine::encoder_head(const Ctx& c, const FullDimSegs& segs, int B, int T50, float* enc_out) {
    const Model& m = *model_;
    const Config& cf = m.cfg();
    const int Tp = (T50 + 1) / 2, Dmax = cf.dmax;
    float* dsd = c.arena->take<float>((int64_t)B * Tp * Dmax);
    downsample_full(c, segs, m.w("encoder.downsample_output.bias"), dsd, B, T50, Dmax, 2);
    if (!enc_out) enc_out = c.arena->take<float>((int64_t)B * Tp * cf.enc_dim());
    if (cf.ctc) {
        linear(c, dsd, Dmax, m.w("ctc_output.1.weight"), m.w("ctc_output.1.bias"), enc_out, cf.V, B * Tp, Dmax, cf.V);
        log_softmax_rows(c, enc_out, B * Tp, cf.V);
    } else {
        linear(c, dsd, Dmax, m.w("joiner.encoder_proj.weight"), m.w("joiner.encoder_proj.bias"), enc_out, cf.J, B * Tp, Dmax, cf.J);
    }
    return enc_out;
}

float* Engine::encoder_forward(const Ctx& c, const float* x, int B, int T, int* Tp, int tap, float** tap_ptr, int* tap_rows,
                               int* tap_dim) {
    const Config& cf = model_->cfg();
    if (cf.conformer) return conformer_forward(c, x, B, T, Tp, tap, tap_ptr, tap_rows, tap_dim);
    if (cf.lstm) return lstm_forward(c, x, B, T, Tp, tap, tap_ptr, tap_rows, tap_dim);
    if (cf.zip1) return zip1_forward(c, x, B, T, Tp, tap, tap_ptr, tap_rows, tap_dim);
    Arena& ar = *c.arena;
    int T50 = 0;
    // output first so that everything after it can be rewound
    int T50_pre = (T - 7) / 2;
    K2_REQUIRE(T50_pre > 0, "encoder: %d input frames are too few", T);
    int Tpp = (T50_pre + 1) / 2;
    float* enc_out = ar.take<float>((int64_t)B * Tpp * cf.enc_dim());
    float* x0 = encoder_embed(c, x, B, T, &T50);
    if (tap_rows) *tap_rows = B * T50;
    if (tap == 0) {
        *tap_ptr = x0;
        *tap_dim = cf.dim[0];
        return nullptr;
    }
    FullDimSegs segs;
    if (encoder_stacks(c, x0, B, T50, nullptr, tap, tap_ptr, tap_dim, &segs)) return nullptr;
    *Tp = Tpp;
    return encoder_head(c, segs, B, T50, enc_out);
}

// The decoder outputs of the two contexts every offline greedy search starts from are constants of the model: computed once (by the
// search kernel's own routine), then shared by the t0 pre-pass and every search workgroup (a 70 us single-workgroup launch per
// batch, and two decoder passes at the head of every search workgroup before).
const float* Engine::decoder_start(const Ctx& c) {
    if (c.dry) return d_dec_start_;
    if (!d_dec_start_) {
        float* p = nullptr;
        K2_HIP(hipMalloc(&p, sizeof(float) * 2 * (size_t)model_->cfg().J));
        decoder_start_contexts(c, decjoin(), p);
        K2_HIP(hipStreamSynchronize(c.stream));  // other streams of this engine read it from now on
        d_dec_start_ = p;
    }
    return d_dec_start_;
}

// ---------------------------------------------------------------------------
// greedy search on device
// ---------------------------------------------------------------------------
Engine::SearchExtras Engine::search_device(const Ctx& c, const float* enc, int B, int Tp, const SearchStage& stage, const SearchOut& out) {
    if (stage.align) return align_device(c, enc, Tp, *stage.align, out);
    if (stage.ctc_align) return ctc_align_device(c, enc, B, Tp, *stage.ctc_align, out);
    if (stage.kws) return kws_device(c, enc, Tp, *stage.kws, out);
    if (stage.ctc_kws) return ctc_kws_device(c, enc, Tp, *stage.ctc_kws, out);
    return greedy_device(c, enc, B, Tp, stage.single, out, stage.keep_nbest);
}

Engine::SearchExtras Engine::greedy_device(const Ctx& c, const float* enc, int B, int Tp, bool single, const SearchOut& out, bool keep_nbest) {
    if (model_->cfg().ctc) {
        if (ctc_prefix_ == 0 || single) return ctc_device(c, enc, B, Tp, out);
        SearchExtras ex = ctc_prefix_device(c, enc, B, Tp, model_->cfg().V, nullptr, ctc_prefix_, out, keep_nbest);
        // the collapse's by-products (NumTrailingBlank bookkeeping) stay the first-argmax rule's: the collapse runs into a block of its own
        const SearchExtras gx = ctc_device(c, enc, B, Tp, SearchOut(*c.arena, B, out.max_tokens));
        ex.trail = gx.trail;
        ex.any = gx.any;
        return ex;
    }
    if (beam_ > 0 && !single) return beam_device(c, enc, B, Tp, out, keep_nbest);
    const Config& cf = model_->cfg();
    Arena& ar = *c.arena;
    DecJoinW w = decjoin();
    int* d_t0 = nullptr;
    if (!c.dry) K2_HIP(hipMemsetAsync(out.flag(), 0, sizeof(int), c.stream));
    const float* dec_start = decoder_start(c);
    if (!single && B > 1) {
        // parallel pass under the initial context [-1, blank]: which frame is the batch's first emission?
        const float* dec_a = dec_start;
        const int N = B * Tp;
        float* act = ar.take<float>((int64_t)N * cf.J);
        tanh_add(c, enc, dec_a, 0, act, N, cf.J);
        float* logits = ar.take<float>((int64_t)N * cf.V);
        linear(c, act, cf.J, model_->w("joiner.output_linear.weight"), model_->w("joiner.output_linear.bias"), logits, cf.V, N,
               cf.J, cf.V);
        int* tok = ar.take<int>(N);
        argmax_rows(c, logits, cf.V, N, cf.V, tok);
        d_t0 = ar.take<int>(1);
        first_emit_frame(c, tok, B, Tp, 0, d_t0);
    }
    GreedyArgs a;
    a.enc = enc; a.B = B; a.Tp = Tp; a.t0 = d_t0; a.skip1 = 0;
    a.max_sym = single ? 1000 : INT_MAX;  // OfflineRecognizer.cs:122
    a.tokens = out.tokens(); a.timestamps = out.timestamps(); a.n_tokens = out.counts(); a.max_tokens = out.max_tokens; a.overflow = out.flag();
    a.dec_init = dec_start;
    a.screen_counts = screen_counts();
    // batch path: rounds of whole-chip GEMMs (they interleave with the next batch's encoder instead of pinning CUs for the whole
    // search); the single-stream path (1000-symbol cap, B = 1) keeps the persistent kernel
    if (!single && tunables().search_rounds == 1) greedy_rounds(c, w, model_->w("joiner.output_linear.weight"), a);
    else greedy_loop(c, w, a);
    return {};
}

// ForwardBatchGreedySearchCTC (OfflineRecognizer.cs:366-424): first-index argmax per frame (parallel), then per stream drop
// blanks and repeats.  logp: [B, Tp, V]
Engine::SearchExtras Engine::ctc_device(const Ctx& c, const float* logp, int B, int Tp, const SearchOut& out) {
    const Config& cf = model_->cfg();
    Arena& ar = *c.arena;
    int* tok = ar.take<int>((int64_t)B * Tp);
    SearchExtras ex;
    ex.trail = ar.take<int>(B);
    ex.any = ar.take<int>(B);
    if (!c.dry) K2_HIP(hipMemsetAsync(out.flag(), 0, sizeof(int), c.stream));
    argmax_first_rows(c, logp, cf.V, B * Tp, cf.V, tok);
    ctc_collapse(c, tok, B, Tp, nullptr, out.tokens(), out.timestamps(), out.counts(), out.max_tokens, ex.trail, ex.any, out.flag());
    return ex;
}

// CTC prefix beam search instead of the collapse (set_ctc_prefix(K) selects it for the batch entries; ctc_prefix.hip)
static_assert(kCtcPrefixMaxBeam == kMaxBeam, "the kernel's and the host reference's beam limit are one number");
Engine::SearchExtras Engine::ctc_prefix_device(const Ctx& c, const float* logp, int R, int Tp, int V, const int32_t* n_frames, int beam,
                                               const SearchOut& out, bool keep_nbest) {
    Arena& ar = *c.arena;
    CtcPrefixArgs a;
    a.log_probs = logp; a.R = R; a.Tp = Tp; a.V = V; a.beam = beam;
    a.nodes = ar.take<int4>((int64_t)R * Tp * beam);
    a.tokens = out.tokens(); a.timestamps = out.timestamps(); a.n_tokens = out.counts(); a.max_tokens = out.max_tokens; a.overflow = out.flag();
    SearchExtras ex;
    ex.scores = ar.take<float>(R);
    a.scores = ex.scores;
    if (n_frames) {
        int* d_nf = ar.take<int>(R);
        if (!c.dry) K2_HIP(hipMemcpyAsync(d_nf, n_frames, sizeof(int) * (size_t)R, hipMemcpyHostToDevice, c.stream));
        a.n_frames = d_nf;
    }
    if (nbest_ > 0 && keep_nbest) {
        const int64_t NB = (int64_t)R * nbest_;
        ex.nb.nbest = nbest_;
        ex.nb.tokens = ar.take<long long>(NB * out.max_tokens);
        ex.nb.timestamps = ar.take<int>(NB * out.max_tokens);
        ex.nb.token_log_probs = ar.take<float>(NB * out.max_tokens);
        ex.nb.n_tokens = ar.take<int>(NB);
        ex.nb.scores = ar.take<float>(NB);
        ex.nb.n_hyps = ar.take<int>(R);
        a.nb = ex.nb;
    }
    if (!c.dry) K2_HIP(hipMemsetAsync(out.flag(), 0, sizeof(int), c.stream));
    if (ctc_prefix_biasing_ && (hw_next_ || lm_.states)) {   // (the tables were built for the model's V, which is every caller's V here)
        K2_REQUIRE(V == model_->cfg().V, "internal: the biased prefix search runs over the model's vocabulary");
        CtcPrefixBiasArgs b;
        static_cast<CtcPrefixArgs&>(b) = a;
        b.hw = BeamHwStream{hw_next_, hw_bonus_, hw_pending_};
        b.lm = lm_;
        ctc_prefix_search_biased(c, b);
    } else {
        ctc_prefix_search(c, a);
    }
    return ex;
}

void Engine::set_ctc_prefix_biasing(bool on) { ctc_prefix_biasing_ = on; }

void Engine::ctc_prefix_host(const float* log_probs, int R, int Tp, const int32_t* n_frames, int beam, int nbest, int64_t* tokens, int32_t* timestamps,
                             float* token_log_probs, int32_t* n_tokens, int32_t* n_hyps, float* scores, int max_tokens) {
    const Config& cf = model_->cfg();
    if (!cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "ctc_prefix_beam_search: model_type '%s' has no CTC head", cf.model_type.c_str());
    K2_REQUIRE(log_probs && tokens && timestamps && token_log_probs && n_tokens && n_hyps && scores, "ctc_prefix_beam_search: null argument");
    ctc_prefix_check_args(R, Tp, cf.V, n_frames, beam, nbest, max_tokens);
    struct Restore {
        int& slot; int old;
        ~Restore() { slot = old; }
    } restore{nbest_, nbest_};
    nbest_ = nbest;
    SearchOut out;
    SearchExtras ex;
    run_sized([&](const Ctx& c) {
        float* d_lp = c.arena->take<float>((int64_t)R * Tp * cf.V);
        out = SearchOut(*c.arena, R, max_tokens);
        if (!c.dry) K2_HIP(hipMemcpyAsync(d_lp, log_probs, sizeof(float) * (size_t)R * Tp * cf.V, hipMemcpyHostToDevice, c.stream));
        ex = ctc_prefix_device(c, d_lp, R, Tp, cf.V, n_frames, beam, out, true);
    });
    // (the single result goes to scratch: entry 0 of the list is that result)
    std::vector<int64_t> tok1((size_t)R * max_tokens);
    std::vector<int32_t> ts1((size_t)R * max_tokens), n1((size_t)R);
    finish_tokens(out, ex, tok1.data(), ts1.data(), n1.data());
    const NbestHost& h = last_nbest_;
    K2_REQUIRE(h.B == R && h.N == nbest && h.max_tokens == max_tokens, "internal: the prefix search kept no N-best");
    for (int r = 0; r < R; r++) {
        n_hyps[r] = h.n_hyps[(size_t)r];
        for (int i = 0; i < h.n_hyps[(size_t)r]; i++) {
            const size_t en = (size_t)r * nbest + i, o = en * max_tokens, len = (size_t)h.n_tokens[en];
            if (len) {
                memcpy(tokens + o, h.tokens.data() + o, sizeof(int64_t) * len);
                memcpy(timestamps + o, h.timestamps.data() + o, sizeof(int32_t) * len);
                memcpy(token_log_probs + o, h.token_log_probs.data() + o, sizeof(float) * len);
            }
            n_tokens[en] = (int32_t)len;
            scores[en] = h.scores[en];
        }
    }
}

// the prefix search resumed from carried prefixes (streaming chunk; CtcPrefixResumeLayout{K, Tc} blocks)
static_assert(kCtcPrefixHashSeed != 0, "the empty prefix's hash is the seed");
void Engine::ctc_prefix_chunk_host(const float* log_probs, int B, int Tc, const int32_t* n_frames, int K, const int* in, int* out) {
    ctc_prefix_chunk_impl(log_probs, B, Tc, n_frames, K, in, out, nullptr);
}
void Engine::ctc_prefix_chunk_host_bias(const float* log_probs, int B, int Tc, const int32_t* n_frames, int K, const int* in, int* out,
                                        const CtcPrefixBiasIO& bias) {
    K2_REQUIRE(bias.graphs && bias.side_in && bias.side_out, "ctc_prefix_beam_search_chunk: null side block");
    ctc_prefix_chunk_impl(log_probs, B, Tc, n_frames, K, in, out, &bias);
}
void Engine::ctc_prefix_chunk_impl(const float* log_probs, int B, int Tc, const int32_t* n_frames, int K, const int* in, int* out,
                                   const CtcPrefixBiasIO* bias) {
    const Config& cf = model_->cfg();
    if (!cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "ctc_prefix_beam_search_chunk: model_type '%s' has no CTC head", cf.model_type.c_str());
    K2_REQUIRE(log_probs && in && out, "ctc_prefix_beam_search_chunk: null argument");
    const CtcPrefixResumeLayout L{K, Tc};
    ctc_prefix_chunk_check_args(B, Tc, cf.V, n_frames, K, in, L.in_ints(), L.in_e(), L.in_rel());
    // ONE upload [log_probs | in blocks | n_frames | biasing: side in blocks, graphs | status] and ONE download [status | out blocks |
    // biasing: side out blocks]
    const CtcPrefixResumeBiasLayout SL{K};
    const int64_t nb_lp = (int64_t)sizeof(float) * B * Tc * cf.V, nb_in = (int64_t)sizeof(int) * B * L.in_ints(), nb_nf = (int64_t)sizeof(int) * B,
                  nb_out = (int64_t)sizeof(int) * B * L.out_ints();
    const int64_t nb_si = bias ? (int64_t)sizeof(int) * B * SL.in_ints() : 0, nb_g = bias ? (int64_t)sizeof(BeamHwStream) * B : 0,
                  nb_so = bias ? (int64_t)sizeof(int) * B * SL.out_ints() : 0;
    const int64_t o_in = align_up(nb_lp, 16), o_nf = align_up(o_in + nb_in, 16), o_si = align_up(o_nf + nb_nf, 16), o_g = align_up(o_si + nb_si, 16),
                  o_st = align_up(o_g + nb_g, 16), in_bytes = o_st + 16;
    K2_HIP(hipSetDevice(device_));
    char* stage = static_cast<char*>(pinned_in(in_bytes));
    memcpy(stage, log_probs, (size_t)nb_lp);
    memcpy(stage + o_in, in, (size_t)nb_in);
    if (n_frames) memcpy(stage + o_nf, n_frames, (size_t)nb_nf);
    if (bias) {
        memcpy(stage + o_si, bias->side_in, (size_t)nb_si);
        memcpy(stage + o_g, bias->graphs, (size_t)nb_g);
    }
    memset(stage + o_st, 0, 16);
    int* d_st = nullptr;
    run_sized([&](const Ctx& c) {
        char* d = c.arena->take<char>(in_bytes + nb_out + nb_so);
        d_st = reinterpret_cast<int*>(d + o_st);
        if (!c.dry) K2_HIP(hipMemcpyAsync(d, stage, (size_t)in_bytes, hipMemcpyHostToDevice, c.stream));
        CtcPrefixResumeBiasArgs a;
        a.log_probs = reinterpret_cast<const float*>(d); a.B = B; a.Tc = Tc; a.V = cf.V; a.beam = K;
        a.n_frames = n_frames ? reinterpret_cast<const int*>(d + o_nf) : nullptr;
        a.nodes = c.arena->take<int4>((int64_t)B * Tc * K);
        a.in = reinterpret_cast<const int*>(d + o_in);
        a.out = reinterpret_cast<int*>(d + in_bytes);
        a.status = d_st;
        if (bias) {
            a.hw_streams = reinterpret_cast<const BeamHwStream*>(d + o_g);
            a.side_in = reinterpret_cast<const int*>(d + o_si);
            a.side_out = reinterpret_cast<int*>(d + in_bytes + nb_out);
            if (bias->lm) a.lm = lm_;
            ctc_prefix_resume_biased(c, a);
        } else {
            ctc_prefix_resume(c, a);   // (no stream of the call is biased: the plain launch, unchanged)
        }
    });
    char* pin = static_cast<char*>(pinned(16 + nb_out + nb_so));
    K2_HIP(hipMemcpyAsync(pin, d_st, (size_t)(16 + nb_out + nb_so), hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
    if (*reinterpret_cast<int*>(pin)) failf(K2HIP_ERR_INVALID, "ctc_prefix_beam_search_chunk: an in block contradicts itself (its relations name tokens the chunk cannot walk)");
    memcpy(out, pin + 16, (size_t)nb_out);
    if (bias) memcpy(bias->side_out, pin + 16 + nb_out, (size_t)nb_so);
}

// modified beam search instead of the greedy loop (set_beam(K) selects it for the fused / operator entry points)
Engine::SearchExtras Engine::beam_device(const Ctx& c, const float* enc, int B, int Tp, const SearchOut& out, bool keep_nbest) {
    BeamArgs a;
    a.enc = enc; a.out_w = model_->w("joiner.output_linear.weight");
    a.dproj_w = model_->w("joiner.decoder_proj.weight");
    a.B = B; a.Tp = Tp; a.beam = beam_;
    a.tokens = out.tokens(); a.timestamps = out.timestamps(); a.n_tokens = out.counts(); a.max_tokens = out.max_tokens; a.overflow = out.flag();
    SearchExtras ex;
    ex.scores = c.arena->take<float>(B);
    a.scores = ex.scores;
    a.hw_next = hw_next_; a.hw_bonus = hw_bonus_; a.hw_pending = hw_pending_;
    a.lm = lm_;
    if (keep_nbest && rnn_lm_fusion_active()) {   // (the pipelined route and recognize_long keep no list: they ignore the switch)
        a.nlm.dev = rnn_dev_;
        a.nlm.scale = rnn_fuse_scale_;
        a.lodr = lodr_;   // (LODR acts only where the neural LM does)
    }
    if (nbest_ > 0 && keep_nbest) {
        const int64_t NB = (int64_t)B * nbest_;
        ex.nb.nbest = nbest_;
        ex.nb.tokens = c.arena->take<long long>(NB * out.max_tokens);
        ex.nb.timestamps = c.arena->take<int>(NB * out.max_tokens);
        ex.nb.token_log_probs = c.arena->take<float>(NB * out.max_tokens);
        ex.nb.n_tokens = c.arena->take<int>(NB);
        ex.nb.scores = c.arena->take<float>(NB);
        ex.nb.n_hyps = c.arena->take<int>(B);
        a.nb = ex.nb;
        a.keep_yp = true;
    }
    if (tunables().beam_trace) {
        ex.trace = c.arena->take<int>((int64_t)B * Tp * (2 * beam_ + 1));
        a.trace = ex.trace;
        ex.trace_B = B; ex.trace_Tp = Tp; ex.trace_K = beam_;
    }
    beam_search(c, decjoin(), a);
    return ex;
}

// modified beam search resumed from saved hypotheses (streaming chunk; BeamResumeLayout{K, Tp} blocks on the device)
void Engine::beam_resume_device(const Ctx& c, const float* enc, int B, int Tp, int K, const int* d_in, int* d_out, int* d_overflow,
                                const BeamHwIO* hw, const NlmStreamIO* d_nlm) {
    BeamArgs a;
    a.enc = enc; a.out_w = model_->w("joiner.output_linear.weight");
    a.dproj_w = model_->w("joiner.decoder_proj.weight");
    a.B = B; a.Tp = Tp; a.beam = K;
    a.tokens = nullptr; a.timestamps = nullptr; a.n_tokens = nullptr; a.scores = nullptr; a.max_tokens = 0;
    a.overflow = d_overflow;
    a.rin = d_in; a.rout = d_out;
    if (hw) {
        a.hw_streams = hw->graphs; a.st_in = hw->st_in; a.st_out = hw->st_out;
        if (hw->lm) {
            a.lm = lm_;
            a.lst_in = hw->st_in + (size_t)B * K;
            a.lst_out = hw->st_out + (size_t)B * K;
        }
        if (hw->lodr && d_nlm) {   // (the last plane of the side blocks)
            a.lodr = lodr_;
            a.dst_in = hw->st_in + (size_t)B * K * (hw->planes() - 1);
            a.dst_out = hw->st_out + (size_t)B * K * (hw->planes() - 1);
        }
    }
    if (d_nlm) {   // neural LM shallow fusion carried across chunks: the streams' state blocks (staged with the in blocks)
        a.nlm.dev = rnn_dev_;
        a.nlm.scale = rnn_fuse_scale_;
        a.nlm_io = d_nlm;
    }
    d_yp_ = nullptr;
    if (yp_host_) {
        yp_floats_ = (size_t)B * K * Tp;
        d_yp_ = c.arena->take<float>((int64_t)yp_floats_);
        a.yp_out = d_yp_;
        a.keep_yp = true;
    }
    beam_search(c, decjoin(), a);
}
void Engine::fetch_beam_yp() {
    if (yp_host_ && d_yp_) K2_HIP(copy_blocking(yp_host_, d_yp_, sizeof(float) * yp_floats_, hipMemcpyDeviceToHost));
    d_yp_ = nullptr;
}

void Engine::beam_chunk_host(const float* enc, int B, int Tp, int K, const int* beam_in, int* beam_out) {
    beam_chunk_impl(enc, B, Tp, K, beam_in, beam_out, nullptr);
}
void Engine::beam_chunk_host_hw(const float* enc, int B, int Tp, int K, const int* beam_in, int* beam_out, const BeamHwIO& hw) {
    beam_chunk_impl(enc, B, Tp, K, beam_in, beam_out, &hw);
}
void Engine::beam_chunk_impl(const float* enc, int B, int Tp, int K, const int* beam_in, int* beam_out, const BeamHwIO* hw) {
    K2_REQUIRE(B > 0 && Tp > 0, "beam chunk: bad shape B=%d T'=%d", B, Tp);
    K2_REQUIRE(K >= 1 && K <= kMaxBeam, "beam chunk: beam %d out of range [1,%d]", K, kMaxBeam);
    const Config& cf = model_->cfg();
    K2_REQUIRE(!cf.ctc, "beam chunk: a CTC model has no transducer search");
    const BeamResumeLayout L{K, Tp};
    // ONE upload [enc | in blocks | hotwords: states in, graphs] and ONE download [flag | out blocks | hotwords: states out]
    const int64_t nb_enc = (int64_t)sizeof(float) * B * Tp * cf.J, nb_in = (int64_t)sizeof(int) * B * L.in_ints(),
                  nb_out = (int64_t)sizeof(int) * B * L.out_ints();
    const int64_t nb_st = hw ? (int64_t)sizeof(int) * B * K * hw->planes() : 0, nb_g = hw ? (int64_t)sizeof(BeamHwStream) * B : 0;
    // (an active streaming neural LM fusion: the streams' block-pointer table rides behind the graphs)
    const NlmStreamIO* nlm_io = nlm_io_host_;
    K2_REQUIRE(!nlm_io || rnn_lm_stream_fusion_active(), "beam chunk: state blocks without an active streaming neural LM fusion");
    const int64_t nb_nl = nlm_io ? (int64_t)sizeof(NlmStreamIO) * B : 0;
    const int64_t o_in = align_up(nb_enc, 16), o_st = align_up(o_in + nb_in, 16), o_g = align_up(o_st + nb_st, 16),
                  o_nl = align_up(o_g + nb_g, 16), o_ovf = align_up(o_nl + nb_nl, 16), in_bytes = o_ovf + 16;
    K2_HIP(hipSetDevice(device_));
    char* stage = static_cast<char*>(pinned_in(in_bytes));
    memcpy(stage, enc, (size_t)nb_enc);
    memcpy(stage + o_in, beam_in, (size_t)nb_in);
    if (hw) {
        memcpy(stage + o_st, hw->st_in, (size_t)nb_st);
        memcpy(stage + o_g, hw->graphs, (size_t)nb_g);
    }
    if (nlm_io) memcpy(stage + o_nl, nlm_io, (size_t)nb_nl);
    memset(stage + o_ovf, 0, 16);
    int* d_ovf = nullptr;
    run_sized([&](const Ctx& c) {
        char* d = c.arena->take<char>(in_bytes + nb_out + nb_st);
        d_ovf = reinterpret_cast<int*>(d + o_ovf);
        if (!c.dry) K2_HIP(hipMemcpyAsync(d, stage, (size_t)in_bytes, hipMemcpyHostToDevice, c.stream));
        const BeamHwIO dhw{reinterpret_cast<const BeamHwStream*>(d + o_g), reinterpret_cast<const int*>(d + o_st),
                           reinterpret_cast<int*>(d + in_bytes + nb_out), hw && hw->lm, hw && hw->lodr};
        beam_resume_device(c, reinterpret_cast<const float*>(d), B, Tp, K, reinterpret_cast<const int*>(d + o_in),
                           reinterpret_cast<int*>(d + in_bytes), d_ovf, hw ? &dhw : nullptr,
                           nlm_io ? reinterpret_cast<const NlmStreamIO*>(d + o_nl) : nullptr);
    });
    char* pin = static_cast<char*>(pinned(16 + nb_out + nb_st));
    K2_HIP(hipMemcpyAsync(pin, d_ovf, (size_t)(16 + nb_out + nb_st), hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
    if (*reinterpret_cast<int*>(pin)) failf(K2HIP_ERR_HIP, "beam chunk: a hypothesis outgrew its buffer");
    memcpy(beam_out, pin + 16, (size_t)nb_out);
    if (hw) memcpy(hw->st_out, pin + 16 + nb_out, (size_t)nb_st);
    fetch_beam_yp();
}

// Back-off of the parted searches.  A search whose column slabs are not co-resident (other handles or processes on the GPU hold the
// CUs) spins to its bound, reports the timeout and is repeated with one workgroup per stream -- correct, but the timeout costs
// milliseconds, every call (four streaming recognizers on one GPU: 12.6 ms per tick against 4.2).  After a timeout the next 4
// searches of this engine go out with one part per stream straight away; each further timeout doubles the span (up to 8192), a parted
// search that comes through clears it.
void Engine::note_search(bool parted, bool timed_out) {
    if (timed_out) {
        if (tunables().test_greedy_timeout == 1) return;   // (the tests' forced timeouts want the next search parted again)
        // exponential back-off from FOUR searches (round 5; 64 before): one timeout while the process warms up -- arenas growing under
        // the first batches, the search kernel's partner slab placed late -- put a whole 20-step run on the one-slab form (the beam-4
        // leg read 16.6 - 16.9 ms per batch in such runs and 14.4 - 14.9 in the others); a GPU that stays contended still reaches
        // 64 after four more timeouts and 8192 after eleven
        one_part_span_ = std::min(std::max(2 * one_part_span_, 4), 8192);
        one_part_left_ = one_part_span_;
    } else if (one_part_left_ > 0) {
        one_part_left_--;
    } else if (parted) {
        one_part_span_ = 0;
    }
}

void Engine::download_search(const SearchOut& out, hipStream_t s, void* pin) {
    K2_HIP(hipMemcpyAsync(pin, out.base, (size_t)out.bytes(), hipMemcpyDeviceToHost, s));
}

void Engine::settle_search(const SearchOut& out, hipStream_t s, GreedyLaunch& rec, void* pin) {
    const int* flag = SearchOut(pin, out.B, out.max_tokens).flag();
    // exchange timeout of a parted search (its workgroups were not co-resident: a shared GPU): the same search once more with one
    // workgroup per stream, which waits for nobody.  Its arena still holds the encoder output and the search's inputs.
    const bool mine = rec.valid && rec.a.overflow == out.flag();
    note_search(mine, *flag == 2 && mine);
    if (*flag == 2 && mine) {
        greedy_relaunch_one_part(s, rec);
        search_retries_++;
        download_search(out, s, pin);
        K2_HIP(hipStreamSynchronize(s));
    }
    rec.valid = false;
    if (*flag == 2) failf(K2HIP_ERR_HIP, "greedy search: the vocabulary-parallel exchange timed out (a workgroup never arrived)");
    if (*flag) failf(K2HIP_ERR_CAPACITY, "a stream emitted more than max_tokens=%d symbols", out.max_tokens);
}

void Engine::finish_tokens(const SearchOut& out, const SearchExtras& ex, int64_t* tokens, int32_t* ts, int32_t* n_tokens) {
    const int B = out.B, max_tokens = out.max_tokens;
    const SearchOut host(pinned(out.bytes()), B, max_tokens);
    download_search(out, stream_, host.base);
    K2_HIP(hipEventRecord(ev_[5], stream_));
    K2_HIP(hipStreamSynchronize(stream_));
    settle_search(out, stream_, last_greedy_, host.base);
    host.copy_out(tokens, ts, n_tokens);
    auto fetch = [](auto& dst, const auto* src, size_t n) {
        dst.resize(n);
        K2_HIP(copy_blocking(dst.data(), src, sizeof(*src) * n, hipMemcpyDeviceToHost));
    };
    if (ex.trail) {
        fetch(last_trail_, ex.trail, (size_t)B);
        fetch(last_any_, ex.any, (size_t)B);
    }
    if (ex.scores) fetch(last_scores_, ex.scores, (size_t)B);
    if (ex.align_lp) {
        fetch(last_align_lp_, ex.align_lp, (size_t)B * max_tokens);
        fetch(last_align_scores_, ex.align_scores, (size_t)B * 2);
    }
    if (ex.align_end) fetch(last_align_end_, ex.align_end, (size_t)B * max_tokens);
    if (ex.kws_a) {
        fetch(last_kws_start_, ex.kws_start, (size_t)B * max_tokens);
        fetch(last_kws_sum_, ex.kws_sum, (size_t)B * max_tokens);
        fetch(last_kws_a_, ex.kws_a, (size_t)ex.kws_states);
        fetch(last_kws_st_, ex.kws_st, (size_t)ex.kws_states);
    }
    NbestHost& h = last_nbest_;
    h.B = 0;
    if (ex.nb.tokens) {
        const size_t NB = (size_t)B * ex.nb.nbest;
        h.B = B; h.N = ex.nb.nbest; h.max_tokens = max_tokens;
        fetch(h.tokens, reinterpret_cast<const int64_t*>(ex.nb.tokens), NB * max_tokens);
        fetch(h.timestamps, ex.nb.timestamps, NB * max_tokens);
        fetch(h.token_log_probs, ex.nb.token_log_probs, NB * max_tokens);
        fetch(h.n_tokens, ex.nb.n_tokens, NB);
        fetch(h.scores, ex.nb.scores, NB);
        fetch(h.n_hyps, ex.nb.n_hyps, (size_t)B);
    }
    if (ex.trace) {
        last_trace_shape_[0] = ex.trace_B; last_trace_shape_[1] = ex.trace_Tp; last_trace_shape_[2] = ex.trace_K;
        fetch(last_beam_trace_, ex.trace, (size_t)ex.trace_B * ex.trace_Tp * (2 * ex.trace_K + 1));
    }
}

Engine::SearchExtras Engine::encode_and_search(const Ctx& c, const float* d_x, int B, int T, const SearchStage& stage, const SearchOut& out) {
    if (!c.dry) K2_HIP(hipEventRecord(ev_[2], c.stream));
    int Tp = 0;
    float* enc = encoder_forward(c, d_x, B, T, &Tp, -1, nullptr, nullptr, nullptr);
    if (!c.dry) K2_HIP(hipEventRecord(ev_[3], c.stream));
    SearchExtras ex = search_device(c, enc, B, Tp, stage, out);
    if (!c.dry) K2_HIP(hipEventRecord(ev_[4], c.stream));
    return ex;
}

void Engine::fill_timing(bool fbank_leg, bool pad_leg) {
    auto el = [&](int a, int b) { float ms = 0; (void)hipEventElapsedTime(&ms, ev_[a], ev_[b]); return ms; };
    timing_.fbank_ms = fbank_leg ? el(0, 1) : 0;   // (from host samples it includes their H2D copy)
    timing_.pad_ms = pad_leg ? el(1, 2) : 0;
    timing_.encoder_ms = el(pad_leg ? 2 : 0, 3);
    timing_.greedy_ms = el(3, 4);
    timing_.d2h_ms = el(4, 5);
    timing_.total_ms = el(0, 5);
}

// ---------------------------------------------------------------------------
// operator-level entry points
// ---------------------------------------------------------------------------
FbankArgs Engine::fbank_args(const float* src, int64_t n, int64_t stride, int n_utts, int64_t nf, float* dst) const {
    const FbankOpts& f = model_->cfg().fbank;
    FbankArgs a{src, n, stride, n_utts, nf, dst, model_->d_window, model_->d_melw, f.frame_len, f.frame_shift, f.preemph, f.input_scale, f.remove_dc};
    a.melrange = model_->d_melrange;
    return a;
}

void Engine::fbank_host(const float* samples, int64_t n, float* feats, int64_t cap_frames, int64_t* n_frames) {
    const FbankOpts& f = model_->cfg().fbank;
    int64_t nf = fbank_num_frames(n);
    if (nf > cap_frames) failf(K2HIP_ERR_CAPACITY, "fbank: %lld frames exceed capacity %lld", (long long)nf, (long long)cap_frames);
    *n_frames = nf;
    if (nf == 0) return;
    float* d_out = nullptr;
    run_sized([&](const Ctx& c) {
        float* d_s = c.arena->take<float>(n);
        d_out = c.arena->take<float>(nf * f.num_bins);
        if (!c.dry) K2_HIP(hipMemcpyAsync(d_s, samples, sizeof(float) * n, hipMemcpyHostToDevice, c.stream));
        fbank(c, fbank_args(d_s, n, n, 1, nf, d_out));
    });
    K2_HIP(hipMemcpyAsync(feats, d_out, sizeof(float) * nf * f.num_bins, hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
}

void Engine::fbank_host_batch(const float* samples, int64_t n, int n_utts, float* feats, int64_t nf) {
    const FbankOpts& f = model_->cfg().fbank;
    K2_REQUIRE(nf == fbank_num_frames(n) && nf > 0 && n_utts > 0, "fbank_host_batch: bad shape");
    // both directions go through the pinned staging buffer: from pageable memory each copy is a synchronous staged transfer,
    // which made a 128-stream AddSamples round cost as much as a tenth of a chunk step
    const size_t nb_in = sizeof(float) * (size_t)n * n_utts, nb_out = sizeof(float) * (size_t)nf * f.num_bins * n_utts;
    char* pin = static_cast<char*>(pinned((int64_t)(nb_in + nb_out + 64)));
    memcpy(pin, samples, nb_in);
    float* d_out = nullptr;
    run_sized([&](const Ctx& c) {
        float* d_s = c.arena->take<float>(n * n_utts);
        d_out = c.arena->take<float>(nf * f.num_bins * n_utts);
        if (!c.dry) K2_HIP(hipMemcpyAsync(d_s, pin, nb_in, hipMemcpyHostToDevice, c.stream));
        fbank(c, fbank_args(d_s, n, n, n_utts, nf, d_out));
    });
    K2_HIP(hipMemcpyAsync(pin + nb_in, d_out, nb_out, hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
    memcpy(feats, pin + nb_in, nb_out);
}

void Engine::fbank_host_gather(const float* const* head, const int64_t* n_head, const float* const* tail, const int64_t* n_tail, int64_t n, int G,
                               float* const* dst, int64_t nf, const int* fifo_slots, const int* fifo_pos, bool defer) {
    const FbankOpts& f = model_->cfg().fbank;
    K2_REQUIRE(nf == fbank_num_frames(n) && nf > 0 && G > 0, "fbank_host_gather: bad shape");
    const size_t nb_in = sizeof(float) * (size_t)n * G, per_out = sizeof(float) * (size_t)nf * f.num_bins, nb_out = per_out * G;
    const bool mirror = fifo_slots && fifo_pos && online_fifo_;
    const size_t nb_idx = mirror ? sizeof(int) * 2 * (size_t)G : 0;
    if (fb_pending_.active) fbank_gather_finish();   // (one outstanding at a time)
    char* pin = static_cast<char*>(defer ? pinned_fb((int64_t)(nb_in + nb_out + nb_idx + 64)) : pinned((int64_t)(nb_in + nb_out + nb_idx + 64)));
    float* w = reinterpret_cast<float*>(pin);
    int* h_idx = reinterpret_cast<int*>(pin + nb_in + nb_out);
    if (mirror) {
        memcpy(h_idx, fifo_slots, sizeof(int) * G);
        memcpy(h_idx + G, fifo_pos, sizeof(int) * G);
    }
    for (int g = 0; g < G; g++) {
        K2_REQUIRE(n_head[g] + n_tail[g] == n, "fbank_host_gather: signal %d has %lld + %lld samples, expected %lld", g, (long long)n_head[g],
                   (long long)n_tail[g], (long long)n);
        if (n_head[g]) memcpy(w + (size_t)g * n, head[g], sizeof(float) * (size_t)n_head[g]);
        if (n_tail[g]) memcpy(w + (size_t)g * n + n_head[g], tail[g], sizeof(float) * (size_t)n_tail[g]);
    }
    float* d_out = nullptr;
    run_sized([&](const Ctx& c) {
        float* d_s = c.arena->take<float>(n * G);
        d_out = c.arena->take<float>(nf * f.num_bins * G);
        if (!c.dry) K2_HIP(hipMemcpyAsync(d_s, pin, nb_in, hipMemcpyHostToDevice, c.stream));
        fbank(c, fbank_args(d_s, n, n, G, nf, d_out));
        if (mirror) {  // the same frames into the streams' device FIFOs: the chunk step then needs no host copy of them
            int* d_idx = c.arena->take<int>(2 * G);
            if (!c.dry) K2_HIP(hipMemcpyAsync(d_idx, h_idx, nb_idx, hipMemcpyHostToDevice, c.stream));
            fifo_append(c, online_fifo_, kFifoFrames, f.num_bins, d_out, d_idx, d_idx + G, G, (int)nf);
        }
    });
    K2_HIP(hipMemcpyAsync(pin + nb_in, d_out, nb_out, hipMemcpyDeviceToHost, stream_));
    if (defer) {
        fb_pending_.dst.assign(dst, dst + G);
        fb_pending_.src = pin + nb_in;
        fb_pending_.per_out = per_out;
        fb_pending_.active = true;
        return;
    }
    K2_HIP(hipStreamSynchronize(stream_));
    for (int g = 0; g < G; g++) memcpy(dst[g], pin + nb_in + (size_t)g * per_out, per_out);
}

// Collect the outstanding download of fbank_host_gather(defer).  Throws if the device work behind it failed: the frames are then
// lost (the destinations keep the zero frames api.cpp reserved for them) and the CALLER must poison the streams that own them --
// nothing may decode those zeros later as if they were audio.  Either way nothing stays outstanding.
void Engine::fbank_gather_finish() {
    if (!fb_pending_.active) return;
    struct Done {
        bool& active;
        ~Done() { active = false; }
    } done{fb_pending_.active};
    K2_HIP(hipStreamSynchronize(stream_));   // (returns at once after the step's own synchronisation)
    for (size_t g = 0; g < fb_pending_.dst.size(); g++) memcpy(fb_pending_.dst[g], fb_pending_.src + g * fb_pending_.per_out, fb_pending_.per_out);
}


// ---- input at another sample rate ----------------------------------------------------------------------------------------------------
const Engine::ResampleDev& Engine::resample_dev(const ResamplePlan& p) {
    K2_REQUIRE(p.out_rate == model_->cfg().fbank.sample_rate, "resample: a plan for %d -> %d on a model that takes %d Hz", p.in_rate, p.out_rate,
               model_->cfg().fbank.sample_rate);
    auto it = rs_cache_.find(p.in_rate);
    if (it != rs_cache_.end()) return it->second;
    const size_t nb_w = align_up((int64_t)sizeof(float) * (int64_t)p.w.size(), 16), nb_i = sizeof(int32_t) * (size_t)p.ou;
    std::vector<char> h(nb_w + 2 * nb_i);
    memcpy(h.data(), p.w.data(), sizeof(float) * p.w.size());
    memcpy(h.data() + nb_w, p.first.data(), nb_i);
    memcpy(h.data() + nb_w + nb_i, p.ntaps.data(), nb_i);
    ResampleDev d;
    K2_HIP(hipMalloc(&d.base, h.size()));
    if (hipError_t e = copy_blocking(d.base, h.data(), h.size(), hipMemcpyHostToDevice); e != hipSuccess) {
        (void)hipFree(d.base);
        K2_HIP(e);
    }
    d.w = reinterpret_cast<const float*>(d.base);
    d.first = reinterpret_cast<const int*>(d.base + nb_w);
    d.ntaps = d.first + p.ou;
    return rs_cache_.emplace(p.in_rate, d).first->second;
}

ResampleRow Engine::resample_row(const ResamplePlan* p, const float* head, int64_t n_head, const float* tail, int64_t n_tail, int64_t x0, int64_t k0,
                                 int64_t n_out, int dst_row) {
    ResampleRow r;
    r.head = head; r.n_head = n_head; r.tail = tail; r.n_tail = n_tail;
    r.dst_row = dst_row;
    if (!p) return r;
    const ResampleDev& d = resample_dev(*p);
    r.x0 = x0; r.k0 = k0; r.n_out = n_out; r.wmax = p->wmax;
    r.w = d.w; r.first = d.first; r.ntaps = d.ntaps;
    r.iu = p->iu; r.ou = p->ou; r.max_taps = p->max_taps;
    return r;
}

void Engine::resample_host(const ResampleJob* jobs, int G) {
    K2_REQUIRE(jobs && G > 0, "resample: empty call");
    K2_HIP(hipSetDevice(device_));
    // the staged inputs back to back, every signal on a 16-byte boundary; the outputs as rows of the longest
    std::vector<int64_t> in_off((size_t)G);
    int64_t n_in = 0, nmax = 1;
    for (int g = 0; g < G; g++) {
        const ResampleJob& j = jobs[g];
        K2_REQUIRE(j.plan && j.n_head >= 0 && j.n_tail >= 0 && j.n_out >= 0 && (j.n_out == 0 || j.out), "resample: signal %d: bad arguments", g);
        in_off[(size_t)g] = n_in;
        n_in += (j.n_head + j.n_tail + 3) & ~(int64_t)3;
        nmax = std::max(nmax, j.n_out);
    }
    nmax = (nmax + 3) & ~(int64_t)3;
    const int64_t nb_in = (int64_t)sizeof(float) * n_in, nb_rows = align_up((int64_t)sizeof(ResampleRow) * G, 16), nb_out = (int64_t)sizeof(float) * G * nmax;
    char* pin = static_cast<char*>(pinned_in(nb_in + nb_rows + nb_out + 64));
    float* h_in = reinterpret_cast<float*>(pin);
    ResampleRow* h_rows = reinterpret_cast<ResampleRow*>(pin + nb_in);
    for (int g = 0; g < G; g++) {
        const ResampleJob& j = jobs[g];
        float* x = h_in + in_off[(size_t)g];
        if (j.n_head) memcpy(x, j.head, sizeof(float) * (size_t)j.n_head);
        if (j.n_tail) memcpy(x + j.n_head, j.tail, sizeof(float) * (size_t)j.n_tail);
    }
    float* d_out = nullptr;
    run_sized([&](const Ctx& c) {
        char* d_in = c.arena->take<char>(nb_in + nb_rows);
        d_out = c.arena->take<float>((int64_t)G * nmax);
        for (int g = 0; g < G; g++) {   // (the rows name device addresses: the arena's, the same in both passes once it is sized)
            const ResampleJob& j = jobs[g];
            h_rows[g] = resample_row(j.plan, c.dry ? nullptr : reinterpret_cast<const float*>(d_in) + in_off[(size_t)g], j.n_head + j.n_tail, nullptr, 0, j.x0, j.k0,
                                     j.n_out, g);
        }
        if (!c.dry) K2_HIP(hipMemcpyAsync(d_in, pin, (size_t)(nb_in + nb_rows), hipMemcpyHostToDevice, c.stream));
        resample_gather(c, h_rows, reinterpret_cast<const ResampleRow*>(d_in + nb_in), G, d_out, G, nmax);
    });
    K2_HIP(hipMemcpyAsync(pin + nb_in + nb_rows, d_out, (size_t)nb_out, hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
    for (int g = 0; g < G; g++)
        if (jobs[g].n_out) memcpy(jobs[g].out, pin + nb_in + nb_rows + sizeof(float) * (size_t)g * (size_t)nmax, sizeof(float) * (size_t)jobs[g].n_out);
}

void Engine::pad_host(const float* const* speech, const int64_t* n_floats, int B, int tail, float* out, int64_t cap, int64_t* Lout) {
    K2_REQUIRE(B > 0, "pad: empty batch");
    int64_t mx = 0, total = 0;
    for (int b = 0; b < B; b++) {
        K2_REQUIRE(n_floats[b] >= 0 && (speech[b] || n_floats[b] == 0), "pad: stream %d has no features", b);
        mx = std::max(mx, n_floats[b]);
        total += n_floats[b];
    }
    int64_t L = mx + 80 * (int64_t)tail;  // PadHelper.cs:22 (80 is hard-coded there)
    *Lout = L;
    if ((int64_t)B * L > cap) failf(K2HIP_ERR_CAPACITY, "pad: need %lld floats, capacity %lld", (long long)B * L, (long long)cap);
    float* d_out = nullptr;
    std::vector<long long> off(B), len(B);
    run_sized([&](const Ctx& c) {
        float* d_packed = c.arena->take<float>(total);
        long long* d_off = c.arena->take<long long>(B);
        long long* d_len = c.arena->take<long long>(B);
        d_out = c.arena->take<float>((int64_t)B * L);
        if (!c.dry) {
            long long o = 0;
            for (int b = 0; b < B; b++) {
                off[b] = o; len[b] = n_floats[b];
                if (n_floats[b]) K2_HIP(hipMemcpyAsync(d_packed + o, speech[b], sizeof(float) * n_floats[b], hipMemcpyHostToDevice, c.stream));
                o += n_floats[b];
            }
            K2_HIP(hipMemcpyAsync(d_off, off.data(), sizeof(long long) * B, hipMemcpyHostToDevice, c.stream));
            K2_HIP(hipMemcpyAsync(d_len, len.data(), sizeof(long long) * B, hipMemcpyHostToDevice, c.stream));
        }
        pad_logfloor(c, d_packed, d_off, d_len, d_out, B, L);
    });
    K2_HIP(hipMemcpyAsync(out, d_out, sizeof(float) * (size_t)B * L, hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
}

void Engine::encoder_host(const float* x, int B, int T, float* enc_out, int64_t cap, int* Tp) {
    K2_REQUIRE(B > 0 && T > 0, "encoder: bad shape B=%d T=%d", B, T);
    int tp = encoder_out_frames(T);
    K2_REQUIRE(tp > 0, "encoder: %d input frames are too few", T);
    const int J = model_->cfg().enc_dim(), feat = model_->cfg().feat;
    if ((int64_t)B * tp * J > cap) failf(K2HIP_ERR_CAPACITY, "encoder: output needs %lld floats", (long long)B * tp * J);
    float* d_enc = nullptr;
    run_sized([&](const Ctx& c) {
        float* d_x = c.arena->take<float>((int64_t)B * T * feat);
        if (!c.dry) K2_HIP(hipMemcpyAsync(d_x, x, sizeof(float) * (size_t)B * T * feat, hipMemcpyHostToDevice, c.stream));
        int t2 = 0;
        d_enc = encoder_forward(c, d_x, B, T, &t2, -1, nullptr, nullptr, nullptr);
    });
    K2_HIP(hipMemcpyAsync(enc_out, d_enc, sizeof(float) * (size_t)B * tp * J, hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
    *Tp = tp;
}

void Engine::encoder_tap_host(const float* x, int B, int T, int tap, float* out, int64_t cap, int64_t* n) {
    K2_REQUIRE(B > 0 && T > 0, "encoder: bad shape B=%d T=%d", B, T);
    const int feat = model_->cfg().feat;
    float* tp = nullptr;
    int rows = 0, dim = 0;
    run_sized([&](const Ctx& c) {
        float* d_x = c.arena->take<float>((int64_t)B * T * feat);
        if (!c.dry) K2_HIP(hipMemcpyAsync(d_x, x, sizeof(float) * (size_t)B * T * feat, hipMemcpyHostToDevice, c.stream));
        int t2 = 0;
        tp = nullptr;
        dim = 0;
        encoder_forward(c, d_x, B, T, &t2, tap, &tp, &rows, &dim);
        K2_REQUIRE(dim > 0, "encoder tap %d does not exist", tap);
    });
    int64_t cnt = (int64_t)rows * dim;
    if (cnt > cap) failf(K2HIP_ERR_CAPACITY, "tap needs %lld floats", (long long)cnt);
    K2_HIP(hipMemcpyAsync(out, tp, sizeof(float) * (size_t)cnt, hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
    *n = cnt;
}

void Engine::decoder_host(const int64_t* y, int N, float* dec_out) {
    K2_REQUIRE(N > 0, "decoder: N=%d", N);
    const Config& cf = model_->cfg();
    std::vector<long long> hy((size_t)N * 2);
    for (int i = 0; i < N; i++) {
        // DecoderProj(null) -> [-1, blank] per row (OfflineProjOfTransducer.cs:97-110)
        hy[2 * i] = y ? y[2 * i] : -1;
        hy[2 * i + 1] = y ? y[2 * i + 1] : K2HIP_BLANK_ID;
        K2_REQUIRE(hy[2 * i] < cf.V && hy[2 * i + 1] < cf.V, "decoder: token id out of range (vocab %d)", cf.V);
    }
    float* d_out = nullptr;
    run_sized([&](const Ctx& c) {
        long long* d_y = c.arena->take<long long>((int64_t)N * 2);
        d_out = c.arena->take<float>((int64_t)N * cf.J);
        if (!c.dry) K2_HIP(hipMemcpyAsync(d_y, hy.data(), sizeof(long long) * hy.size(), hipMemcpyHostToDevice, c.stream));
        decoder(c, decjoin(), d_y, N, d_out);
    });
    K2_HIP(hipMemcpyAsync(dec_out, d_out, sizeof(float) * (size_t)N * cf.J, hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
}

void Engine::joiner_host(const float* enc, const float* dec, int N, float* logits) {
    K2_REQUIRE(N > 0, "joiner: N=%d", N);
    const Config& cf = model_->cfg();
    float* d_l = nullptr;
    run_sized([&](const Ctx& c) {
        float* d_e = c.arena->take<float>((int64_t)N * cf.J);
        float* d_d = c.arena->take<float>((int64_t)N * cf.J);
        float* d_a = c.arena->take<float>((int64_t)N * cf.J);
        d_l = c.arena->take<float>((int64_t)N * cf.V);
        if (!c.dry) {
            K2_HIP(hipMemcpyAsync(d_e, enc, sizeof(float) * (size_t)N * cf.J, hipMemcpyHostToDevice, c.stream));
            K2_HIP(hipMemcpyAsync(d_d, dec, sizeof(float) * (size_t)N * cf.J, hipMemcpyHostToDevice, c.stream));
        }
        tanh_add(c, d_e, d_d, cf.J, d_a, N, cf.J);
        linear(c, d_a, cf.J, model_->w("joiner.output_linear.weight"), model_->w("joiner.output_linear.bias"), d_l, cf.V, N, cf.J, cf.V);
    });
    K2_HIP(hipMemcpyAsync(logits, d_l, sizeof(float) * (size_t)N * cf.V, hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
}

void Engine::greedy_host(const float* enc_out, int B, int Tp, bool single, int64_t* tokens, int32_t* ts, int32_t* n_tokens,
                         int max_tokens) {
    K2_REQUIRE(B > 0 && Tp > 0 && max_tokens > 0, "greedy: bad shape B=%d T'=%d max_tokens=%d", B, Tp, max_tokens);
    K2_REQUIRE(!single || B == 1, "greedy_single: B must be 1");
    search_host(enc_out, B, Tp, SearchStage{single}, tokens, ts, n_tokens, max_tokens);
}

void Engine::search_host(const float* enc_out, int B, int Tp, const SearchStage& stage, int64_t* tokens, int32_t* ts, int32_t* n_tokens,
                         int max_tokens) {
    const int64_t n = (int64_t)B * Tp * model_->cfg().enc_dim();
    SearchOut out;
    SearchExtras ex;
    run_sized([&](const Ctx& c) {
        float* d_e = c.arena->take<float>(n);
        out = SearchOut(*c.arena, stage.rows(B), max_tokens);
        if (!c.dry) K2_HIP(hipMemcpyAsync(d_e, enc_out, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c.stream));
        ex = search_device(c, d_e, B, Tp, stage, out);
    });
    finish_tokens(out, ex, tokens, ts, n_tokens);
}

// ---------------------------------------------------------------------------
// forced alignment and full-sum scoring (align.hip)
// ---------------------------------------------------------------------------
Engine::SearchExtras Engine::align_device(const Ctx& c, const float* enc, int Tp, const AlignPlan& p, const SearchOut& out, float* stay,
                                          float* emit, bool cells, bool dp) {
    K2_REQUIRE(Tp == p.Tp && out.B == p.B, "internal: the align plan was laid out for T'=%d B=%d, the encoder gave T'=%d B=%d", p.Tp, p.B, Tp, out.B);
    const Config& cf = model_->cfg();
    Arena& ar = *c.arena;
    char* d_blob = ar.take<char>((int64_t)p.blob.size());
    AlignArgs a;
    a.enc = enc; a.B = p.B; a.Tp = Tp; a.max_T = p.max_T; a.max_U = p.max_U;
    a.streams = reinterpret_cast<const AlignStream*>(d_blob);
    a.ids = reinterpret_cast<const int*>(d_blob + p.o_ids);
    const long long* d_ctx = reinterpret_cast<const long long*>(d_blob + p.o_ctx);
    float* d_dec = cells ? ar.take<float>((int64_t)p.n_ctx * cf.J) : nullptr;
    a.dec = d_dec;
    a.stay = stay ? stay : ar.take<float>(p.plane_floats);
    a.emit = emit ? emit : ar.take<float>(p.plane_floats);
    if (!c.dry) K2_HIP(hipMemcpyAsync(d_blob, p.blob.data(), p.blob.size(), hipMemcpyHostToDevice, c.stream));
    if (cells) {
        // the decoder table is not consulted: decoder() runs the U + 1 contexts of every stream in one launch
        const DecJoinW w = decjoin();
        decoder(c, w, d_ctx, p.n_ctx, d_dec);
        lattice_logprobs(c, w, a);
    }
    SearchExtras ex;
    if (!dp) return ex;
    a.bp = ar.take<unsigned long long>(p.bp_words);
    ex.align_lp = ar.take<float>((int64_t)p.B * out.max_tokens);
    ex.align_scores = ar.take<float>((int64_t)p.B * 2);
    a.tokens = cells ? out.tokens() : nullptr;
    a.timestamps = out.timestamps(); a.n_tokens = out.counts(); a.max_tokens = out.max_tokens;
    a.token_log_probs = ex.align_lp; a.scores = ex.align_scores;
    if (!c.dry) K2_HIP(hipMemsetAsync(out.flag(), 0, sizeof(int), c.stream));
    lattice_dp(c, a);
    return ex;
}

void Engine::align_copy_out(int rows, const int32_t* lens, const AlignScratch& s, int32_t* timestamps, int32_t* end_frames, float* token_log_probs,
                            float* total, float* best) const {
    for (int r = 0; r < rows; r++) {
        const size_t o = (size_t)r * s.mt, n = (size_t)lens[r];
        if (timestamps && n) memcpy(timestamps + o, s.ts.data() + o, sizeof(int32_t) * n);
        if (end_frames && n) memcpy(end_frames + o, last_align_end_.data() + o, sizeof(int32_t) * n);
        if (token_log_probs && n) memcpy(token_log_probs + o, last_align_lp_.data() + o, sizeof(float) * n);
        if (total) total[r] = last_align_scores_[2 * (size_t)r];
        if (best) best[r] = last_align_scores_[2 * (size_t)r + 1];
    }
}

void Engine::align_host(const float* enc_out, int B, int Tp, const int32_t* n_frames, const int64_t* ids, const int32_t* lens, int32_t* timestamps,
                        float* token_log_probs, float* total, float* best, int max_tokens) {
    K2_REQUIRE(enc_out != nullptr && max_tokens >= 0, "align: bad arguments");
    const AlignPlan p = align_plan(B, Tp, n_frames, ids, lens, max_tokens);
    AlignScratch s(B, max_tokens);
    SearchStage stage;
    stage.align = &p;
    search_host(enc_out, B, Tp, stage, s.tok.data(), s.ts.data(), s.n.data(), s.mt);
    align_copy_out(B, lens, s, timestamps, nullptr, token_log_probs, total, best);
}

void Engine::align_samples(const float* const* samples, const int64_t* n_samples, int B, const int64_t* ids, const int32_t* lens,
                           int32_t* timestamps, float* token_log_probs, float* total, float* best, int max_tokens, int32_t* Tp_out) {
    K2_REQUIRE(samples != nullptr && n_samples != nullptr && B > 0 && max_tokens >= 0, "align_from_samples: bad arguments");
    const Config& cf = model_->cfg();
    if (cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "align: a CTC model has no transducer lattice");
    const int Tp = samples_frames("align_from_samples", samples, n_samples, B);
    const AlignPlan p = align_plan(B, Tp, nullptr, ids, lens, max_tokens);
    AlignScratch s(B, max_tokens);
    SearchStage stage;
    stage.align = &p;
    offline_samples(samples, n_samples, B, stage, s.tok.data(), s.ts.data(), s.n.data(), s.mt, false);
    align_copy_out(B, lens, s, timestamps, nullptr, token_log_probs, total, best);
    if (Tp_out) *Tp_out = Tp;
}

// ---------------------------------------------------------------------------
// keyword spotting: trie Viterbi on the lattice (kws.hip)
// ---------------------------------------------------------------------------
void* Engine::kws_graph_upload(const KeywordGraph& g, KwsGraphDev* out) {
    const Config& cf = model_->cfg();
    if (cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "keyword spotting: a CTC model has no transducer lattice");
    K2_REQUIRE(cf.ctx == 2, "keyword spotting: decoder context size %d (2 is built)", cf.ctx);
    K2_REQUIRE(g.vocab_size() == cf.V, "keyword spotting: the graph was built for vocab_size %d, the model has %d", g.vocab_size(), cf.V);
    const int S = g.num_states();
    const std::vector<int64_t> ctx = g.contexts(2);
    std::vector<long long> hy(ctx.begin(), ctx.end());
    // [dec | parent | depth | kw | bar | child_off | child_tok | child_state], every piece on 16 bytes
    const int64_t nb_dec = align_up((int64_t)sizeof(float) * S * cf.J, 16), nb_s = align_up((int64_t)sizeof(int32_t) * (S + 1), 16);
    char* d = static_cast<char*>(dev_alloc(nb_dec + 7 * nb_s));
    try {
        char* t = d + nb_dec;
        const void* src[7] = {g.parent().data(), g.depth().data(), g.kw().data(), g.bar().data(), g.child_off().data(), g.child_tok().data(),
                              g.child_state().data()};
        const int64_t cnt[7] = {S, S, S, S, S + 1, S - 1, S - 1};
        for (int k = 0; k < 7; k++)
            if (cnt[k] > 0) dev_upload(t + k * nb_s, src[k], 4 * cnt[k]);
        run_sized([&](const Ctx& c) {
            long long* d_y = c.arena->take<long long>((int64_t)S * 2);
            if (!c.dry) K2_HIP(hipMemcpyAsync(d_y, hy.data(), sizeof(long long) * hy.size(), hipMemcpyHostToDevice, c.stream));
            decoder(c, decjoin(), d_y, S, reinterpret_cast<float*>(d));
        });
        K2_HIP(hipStreamSynchronize(stream_));
        out->dec = reinterpret_cast<const float*>(d);
        out->parent = reinterpret_cast<const int*>(t);
        out->depth = reinterpret_cast<const int*>(t + nb_s);
        out->kw = reinterpret_cast<const int*>(t + 2 * nb_s);
        out->bar = reinterpret_cast<const float*>(t + 3 * nb_s);
        out->child_off = reinterpret_cast<const int*>(t + 4 * nb_s);
        out->child_tok = reinterpret_cast<const int*>(t + 5 * nb_s);
        out->child_state = reinterpret_cast<const int*>(t + 6 * nb_s);
        out->S = S;
    } catch (...) {
        try { dev_free(d); } catch (...) {}
        throw;
    }
    return d;
}

Engine::SearchExtras Engine::kws_device(const Ctx& c, const float* enc, int Tp, const KwsPlan& p, const SearchOut& out, float* stay, float* emit,
                                        bool cells, bool dp) {
    K2_REQUIRE(Tp == p.Tp && out.B == p.B && out.max_tokens >= std::max(p.max_T, 1),
               "internal: the keyword plan was laid out for T'=%d B=%d, the encoder gave T'=%d B=%d", p.Tp, p.B, Tp, out.B);
    Arena& ar = *c.arena;
    char* d_blob = ar.take<char>((int64_t)p.blob.size());
    KwsArgs a;
    a.enc = enc; a.B = p.B; a.Tp = Tp; a.max_T = p.max_T; a.max_S = p.max_S;
    a.streams = reinterpret_cast<const KwsStream*>(d_blob);
    a.a_in = reinterpret_cast<const float*>(d_blob + p.o_a);
    a.start_in = reinterpret_cast<const int*>(d_blob + p.o_st);
    a.stay = stay ? stay : ar.take<float>(std::max<long long>(p.plane_floats, 1));
    a.emit = emit ? emit : ar.take<float>(std::max<long long>(p.plane_floats, 1));
    if (!c.dry) K2_HIP(hipMemcpyAsync(d_blob, p.blob.data(), p.blob.size(), hipMemcpyHostToDevice, c.stream));
    if (cells) trie_logprobs(c, decjoin(), a);
    SearchExtras ex;
    if (!dp) return ex;
    const int64_t ne = (int64_t)p.B * out.max_tokens;
    ex.kws_start = ar.take<int>(ne);
    ex.kws_sum = ar.take<float>(ne);
    ex.kws_a = ar.take<float>(p.n_states);
    ex.kws_st = ar.take<int>(p.n_states);
    ex.kws_states = p.n_states;
    a.a_out = ex.kws_a; a.start_out = ex.kws_st;
    a.ev_keyword = out.tokens(); a.ev_end = out.timestamps(); a.n_events = out.counts(); a.max_events = out.max_tokens;
    a.ev_start = ex.kws_start; a.ev_sum = ex.kws_sum;
    if (!c.dry) K2_HIP(hipMemsetAsync(out.flag(), 0, sizeof(int), c.stream));
    trie_dp(c, a);
    return ex;
}

void Engine::kws_collect(const std::vector<int32_t>& state_off, int mt, std::vector<int64_t>&& tok, std::vector<int32_t>&& ts, std::vector<int32_t>&& n,
                         KwsResult* res) const {
    res->mt = mt;
    res->keyword = std::move(tok);
    res->end = std::move(ts);
    res->n = std::move(n);
    res->start = last_kws_start_;
    res->sum = last_kws_sum_;
    res->a = last_kws_a_;
    res->st = last_kws_st_;
    res->state_off = state_off;
}

void Engine::kws_chunk_host(const float* enc_out, int B, int Tc, const KwsIO* io, KwsResult* res) {
    K2_REQUIRE(enc_out != nullptr && res != nullptr, "keyword spotting: bad arguments");
    const KwsPlan p = kws_plan(B, Tc, io, false);
    const int mt = std::max(p.max_T, 1);
    std::vector<int64_t> tok((size_t)B * mt);
    std::vector<int32_t> ts((size_t)B * mt), n((size_t)B);
    SearchStage stage;
    stage.kws = &p;
    search_host(enc_out, B, Tc, stage, tok.data(), ts.data(), n.data(), mt);
    kws_collect(p.state_off, mt, std::move(tok), std::move(ts), std::move(n), res);
}

void Engine::kws_samples(const float* const* samples, const int64_t* n_samples, int B, const KwsIO* io, KwsResult* res, int32_t* Tp_out) {
    K2_REQUIRE(samples != nullptr && n_samples != nullptr && B > 0 && res != nullptr, "spot_keywords_from_samples: bad arguments");
    if (model_->cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "keyword spotting: a CTC model has no transducer lattice");
    const int Tp = samples_frames("spot_keywords_from_samples", samples, n_samples, B);
    const KwsPlan p = kws_plan(B, Tp, io, true);
    std::vector<int64_t> tok((size_t)B * Tp);
    std::vector<int32_t> ts((size_t)B * Tp), n((size_t)B);
    SearchStage stage;
    stage.kws = &p;
    offline_samples(samples, n_samples, B, stage, tok.data(), ts.data(), n.data(), Tp, false);
    kws_collect(p.state_off, Tp, std::move(tok), std::move(ts), std::move(n), res);
    if (Tp_out) *Tp_out = Tp;
}

// ---------------------------------------------------------------------------
// keyword spotting for CTC models: trie Viterbi on the CTC trellis (ctc_kws.hip)
// ---------------------------------------------------------------------------
Engine::SearchExtras Engine::ctc_kws_device(const Ctx& c, const float* logp, int Tp, const CtcKwsPlan& p, const SearchOut& out) {
    K2_REQUIRE(Tp == p.Tp && out.B == p.B && out.max_tokens >= std::max(p.max_T, 1),
               "internal: the CTC keyword plan was laid out for T'=%d B=%d, the encoder gave T'=%d B=%d", p.Tp, p.B, Tp, out.B);
    Arena& ar = *c.arena;
    char* d_blob = ar.take<char>((int64_t)p.blob.size());
    CtcKwsArgs a;
    a.log_probs = logp; a.B = p.B; a.Tp = Tp; a.V = p.V; a.max_T = p.max_T; a.max_S = p.max_S;
    a.streams = reinterpret_cast<const CtcKwsStream*>(d_blob);
    a.v_in = reinterpret_cast<const float*>(d_blob + p.o_v);
    a.st_in = reinterpret_cast<const int*>(d_blob + p.o_st);
    a.tables = reinterpret_cast<const int*>(d_blob + p.o_tab);
    SearchExtras ex;
    const int64_t ne = (int64_t)p.B * out.max_tokens;
    ex.kws_start = ar.take<int>(ne);
    ex.kws_sum = ar.take<float>(ne);
    ex.kws_a = ar.take<float>(2 * (int64_t)p.n_states);
    ex.kws_st = ar.take<int>(2 * (int64_t)p.n_states);
    ex.kws_states = 2 * p.n_states;
    a.v_out = ex.kws_a; a.st_out = ex.kws_st;
    a.ev_keyword = out.tokens(); a.ev_end = out.timestamps(); a.n_events = out.counts(); a.max_events = out.max_tokens;
    a.ev_start = ex.kws_start; a.ev_sum = ex.kws_sum;
    if (!c.dry) {
        K2_HIP(hipMemcpyAsync(d_blob, p.blob.data(), p.blob.size(), hipMemcpyHostToDevice, c.stream));
        K2_HIP(hipMemsetAsync(out.flag(), 0, sizeof(int), c.stream));
    }
    ctc_trie_dp(c, a);
    return ex;
}

void Engine::ctc_kws_chunk_host(const float* log_probs, int B, int Tc, const CtcKwsIO* io, KwsResult* res) {
    K2_REQUIRE(log_probs != nullptr && res != nullptr, "CTC keyword spotting: bad arguments");
    const CtcKwsPlan p = ctc_kws_plan(B, Tc, io, false);
    const int mt = std::max(p.max_T, 1);
    std::vector<int64_t> tok((size_t)B * mt);
    std::vector<int32_t> ts((size_t)B * mt), n((size_t)B);
    SearchStage stage;
    stage.ctc_kws = &p;
    search_host(log_probs, B, Tc, stage, tok.data(), ts.data(), n.data(), mt);
    kws_collect(p.state_off, mt, std::move(tok), std::move(ts), std::move(n), res);
}

void Engine::ctc_kws_samples(const float* const* samples, const int64_t* n_samples, int B, const CtcKwsIO* io, KwsResult* res, int32_t* Tp_out) {
    K2_REQUIRE(samples != nullptr && n_samples != nullptr && B > 0 && res != nullptr, "ctc_spot_keywords_from_samples: bad arguments");
    if (!model_->cfg().ctc) failf(K2HIP_ERR_UNSUPPORTED, "CTC keyword spotting: model_type '%s' has no CTC head", model_->cfg().model_type.c_str());
    const int Tp = samples_frames("ctc_spot_keywords_from_samples", samples, n_samples, B);
    const CtcKwsPlan p = ctc_kws_plan(B, Tp, io, true);
    std::vector<int64_t> tok((size_t)B * Tp);
    std::vector<int32_t> ts((size_t)B * Tp), n((size_t)B);
    SearchStage stage;
    stage.ctc_kws = &p;
    offline_samples(samples, n_samples, B, stage, tok.data(), ts.data(), n.data(), Tp, false);
    kws_collect(p.state_off, Tp, std::move(tok), std::move(ts), std::move(n), res);
    if (Tp_out) *Tp_out = Tp;
}

// ---------------------------------------------------------------------------
// CTC forced alignment and full-sum scoring (ctc_align.hip)
// ---------------------------------------------------------------------------
Engine::SearchExtras Engine::ctc_align_device(const Ctx& c, const float* logp, int R, int Tp, const CtcAlignPlan& p, const SearchOut& out) {
    K2_REQUIRE(Tp == p.Tp && R == p.R && out.B == p.H, "internal: the CTC align plan was laid out for T'=%d R=%d H=%d, the encoder gave T'=%d R=%d H=%d",
               p.Tp, p.R, p.H, Tp, R, out.B);
    Arena& ar = *c.arena;
    char* d_blob = ar.take<char>((int64_t)p.blob.size());
    CtcAlignArgs a;
    a.log_probs = logp; a.Tp = Tp; a.V = model_->cfg().V; a.H = p.H; a.max_T = p.max_T; a.max_U = p.max_U;
    a.targets = reinterpret_cast<const CtcAlignTarget*>(d_blob);
    a.ids = reinterpret_cast<const int*>(d_blob + p.o_ids);
    a.plane = ar.take<float>(p.plane_floats);
    a.bp = ar.take<unsigned long long>(p.bp_words);
    SearchExtras ex;
    ex.align_lp = ar.take<float>((int64_t)p.H * out.max_tokens);
    ex.align_end = ar.take<int>((int64_t)p.H * out.max_tokens);
    ex.align_scores = ar.take<float>((int64_t)p.H * 2);
    a.tokens = out.tokens(); a.timestamps = out.timestamps(); a.n_tokens = out.counts(); a.max_tokens = out.max_tokens;
    a.end_frames = ex.align_end; a.token_log_probs = ex.align_lp; a.scores = ex.align_scores;
    if (!c.dry) {
        K2_HIP(hipMemcpyAsync(d_blob, p.blob.data(), p.blob.size(), hipMemcpyHostToDevice, c.stream));
        K2_HIP(hipMemsetAsync(out.flag(), 0, sizeof(int), c.stream));
    }
    ctc_lattice(c, a);
    return ex;
}

void Engine::ctc_align_host(const float* log_probs, int R, int Tp, const int32_t* n_frames, int H, const int32_t* stream_of, const int64_t* ids,
                            const int32_t* lens, int32_t* timestamps, int32_t* end_frames, float* token_log_probs, float* total, float* best,
                            int max_tokens) {
    K2_REQUIRE(log_probs != nullptr && max_tokens >= 0, "ctc_align: bad arguments");
    const CtcAlignPlan p = ctc_align_plan(R, Tp, n_frames, H, stream_of, ids, lens, max_tokens);
    AlignScratch s(H, max_tokens);
    SearchStage stage;
    stage.ctc_align = &p;
    search_host(log_probs, R, Tp, stage, s.tok.data(), s.ts.data(), s.n.data(), s.mt);
    align_copy_out(H, lens, s, timestamps, end_frames, token_log_probs, total, best);
}

void Engine::ctc_align_samples(const float* const* samples, const int64_t* n_samples, int B, int H, const int32_t* stream_of, const int64_t* ids,
                               const int32_t* lens, int32_t* timestamps, int32_t* end_frames, float* token_log_probs, float* total, float* best,
                               int max_tokens, int32_t* Tp_out) {
    K2_REQUIRE(samples != nullptr && n_samples != nullptr && B > 0 && max_tokens >= 0, "ctc_align_from_samples: bad arguments");
    const Config& cf = model_->cfg();
    if (!cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "ctc_align: model_type '%s' has no CTC head", cf.model_type.c_str());
    const int Tp = samples_frames("ctc_align_from_samples", samples, n_samples, B);
    const CtcAlignPlan p = ctc_align_plan(B, Tp, nullptr, H, stream_of, ids, lens, max_tokens);
    AlignScratch s(H, max_tokens);
    SearchStage stage;
    stage.ctc_align = &p;
    offline_samples(samples, n_samples, B, stage, s.tok.data(), s.ts.data(), s.n.data(), s.mt, false);
    align_copy_out(H, lens, s, timestamps, end_frames, token_log_probs, total, best);
    if (Tp_out) *Tp_out = Tp;
}

// ---------------------------------------------------------------------------
// fused paths
// ---------------------------------------------------------------------------
Engine::OfflineShape Engine::offline_shape(const char* who, int64_t longest, bool from_feats) const {
    const Config& cf = model_->cfg();
    K2_REQUIRE(cf.ctc || cf.J == 512, "offline loops hard-code a 512-wide encoder_out (OfflineRecognizer.cs:103,201); joiner_dim is %d", cf.J);
    OfflineShape s;
    s.longest = longest;
    s.frames = from_feats ? longest / cf.feat : fbank_num_frames(longest);
    K2_REQUIRE(from_feats || s.frames > 0, "%s: %lld samples give no frame", who, (long long)longest);
    s.n_fl = from_feats ? longest : s.frames * cf.feat;
    s.L = s.n_fl + 80 * kTailFrames;  // PadHelper.cs:17,22
    s.T = (int)(s.L / cf.feat);       // OfflineProjOfTransducer.cs:59
    s.Tp = encoder_out_frames(s.T);
    return s;
}

Engine::OfflineShape Engine::samples_shape(const float* const* samples, const int64_t* n_samples, int B) const {
    int64_t nmax = 0;
    for (int b = 0; b < B; b++) {
        const int64_t n = wave_count(b, n_samples[b]);
        K2_REQUIRE(samples[b] != nullptr && fbank_num_frames(n) > 0, "stream %d: %lld samples give no frame", b, (long long)n);
        nmax = std::max(nmax, n);
    }
    return offline_shape("offline_greedy_from_samples", nmax);
}

int Engine::samples_frames(const char* who, const float* const* samples, const int64_t* n_samples, int B) const {
    const OfflineShape sh = samples_shape(samples, n_samples, B);
    K2_REQUIRE(sh.Tp > 0, "%s: %lld samples give no encoder frame", who, (long long)sh.longest);
    return sh.Tp;
}

void Engine::offline_greedy_feats(const float* const* feats, const int64_t* n_floats, int B, bool single, int64_t* tokens,
                                  int32_t* ts, int32_t* n_tokens, int max_tokens) {
    K2_REQUIRE(B > 0 && max_tokens > 0, "offline_greedy: bad B=%d / max_tokens=%d", B, max_tokens);
    K2_REQUIRE(!single || B == 1, "offline_greedy_single: B must be 1");
    int64_t mx = 0, total = 0;
    for (int b = 0; b < B; b++) {
        K2_REQUIRE(feats[b] != nullptr && n_floats[b] > 0, "offline_greedy: stream %d has no features", b);
        mx = std::max(mx, n_floats[b]);
        total += n_floats[b];
    }
    const OfflineShape sh = offline_shape("offline_greedy", mx, true);
    K2_REQUIRE(sh.L % model_->cfg().feat == 0, "offline_greedy: padded length %lld is not a multiple of feature_dim", (long long)sh.L);
    // stage all features in one pinned buffer -> one H2D
    float* pin = static_cast<float*>(pinned(sizeof(float) * total + 16 * B + 64));
    std::vector<long long> off(B), len(B);
    {
        long long o = 0;
        for (int b = 0; b < B; b++) {
            memcpy(pin + o, feats[b], sizeof(float) * n_floats[b]);
            off[b] = o; len[b] = n_floats[b];
            o += n_floats[b];
        }
    }
    SearchOut out;
    SearchExtras ex;
    run_sized([&](const Ctx& c) {
        Arena& ar = *c.arena;
        out = SearchOut(ar, B, max_tokens);
        float* d_packed = ar.take<float>(total);
        long long* d_off = ar.take<long long>(B);
        long long* d_len = ar.take<long long>(B);
        float* d_x = ar.take<float>((int64_t)B * sh.L);
        if (!c.dry) {
            K2_HIP(hipEventRecord(ev_[0], c.stream));
            K2_HIP(hipMemcpyAsync(d_packed, pin, sizeof(float) * total, hipMemcpyHostToDevice, c.stream));
            K2_HIP(hipMemcpyAsync(d_off, off.data(), sizeof(long long) * B, hipMemcpyHostToDevice, c.stream));
            K2_HIP(hipMemcpyAsync(d_len, len.data(), sizeof(long long) * B, hipMemcpyHostToDevice, c.stream));
            K2_HIP(hipEventRecord(ev_[1], c.stream));
        }
        pad_logfloor(c, d_packed, d_off, d_len, d_x, B, sh.L);
        ex = encode_and_search(c, d_x, B, sh.T, SearchStage{single}, out);
    });
    finish_tokens(out, ex, tokens, ts, n_tokens);
    fill_timing(false, true);
}

void Engine::offline_greedy_samples_dev(const float* samples_dev, int64_t n_each, int B, int64_t* tokens, int32_t* ts,
                                        int32_t* n_tokens, int max_tokens) {
    K2_REQUIRE(B > 0 && max_tokens > 0 && samples_dev != nullptr, "offline_greedy_from_samples: bad arguments");
    const OfflineShape sh = offline_shape("offline_greedy_from_samples", n_each);
    SearchOut out;
    SearchExtras ex;
    run_sized([&](const Ctx& c) {
        Arena& ar = *c.arena;
        out = SearchOut(ar, B, max_tokens);
        float* d_feats = ar.take<float>((int64_t)B * sh.n_fl);
        float* d_x = ar.take<float>((int64_t)B * sh.L);
        if (!c.dry) K2_HIP(hipEventRecord(ev_[0], c.stream));
        fbank(c, fbank_args(samples_dev, n_each, n_each, B, sh.frames, d_feats));
        if (!c.dry) K2_HIP(hipEventRecord(ev_[1], c.stream));
        pad_logfloor_dense(c, d_feats, sh.n_fl, d_x, B, sh.L);
        ex = encode_and_search(c, d_x, B, sh.T, SearchStage{}, out);
    });
    finish_tokens(out, ex, tokens, ts, n_tokens);
    fill_timing(true, true);
}

void Engine::offline_greedy_samples(const float* const* samples, const int64_t* n_samples, int B, int64_t* tokens, int32_t* ts,
                                    int32_t* n_tokens, int max_tokens, bool single, bool pinned_src) {
    offline_samples(samples, n_samples, B, SearchStage{single}, tokens, ts, n_tokens, max_tokens, pinned_src);
}

void Engine::offline_samples(const float* const* samples, const int64_t* n_samples, int B, const SearchStage& stage, int64_t* tokens, int32_t* ts,
                             int32_t* n_tokens, int max_tokens, bool pinned_src) {
    // Host samples, any lengths: ONE pinned staging block [B, nmax] (tails zeroed) + the streams' feature offsets / lengths, one H2D,
    // ONE batched fbank launch over nmax samples per stream, then the fused feature path on the device.  A frame i < frames(n_b) of
    // stream b only reads samples below n_b, so the zero tail never reaches a frame that is kept; pad_logfloor takes each stream's
    // own frame count.  (Rounds 1 - 4 ran one fbank round trip per stream here and uploaded the features again.)  This is what
    // OfflineRecognizer.GetResults reaches through k2hip_offline_recognizer_get_results (OfflineStream.cs:43-57 + OfflineRecognizer.cs:85-91).
    // pinned_src: the sample arrays live in pinned host memory (the native OfflineStreams' queues, Engine::host_alloc): no staging block --
    // only the table of pointers and lengths is uploaded, and a gather kernel reads the samples in place over PCIe into the dense [B, nmax]
    // device block (tails zeroed there): the host's 20 MB staging copy and the separate upload of a 32 x 10 s batch become one pass.
    K2_REQUIRE(B > 0 && max_tokens > 0, "offline_greedy_from_samples: bad B=%d / max_tokens=%d", B, max_tokens);
    K2_REQUIRE(!stage.single || B == 1, "offline_greedy_from_samples: the single-stream loop takes one stream");
    K2_HIP(hipSetDevice(device_));   // (the pinned queues' device addresses are asked for below, before run_sized sets it)
    const OfflineShape sh = samples_shape(samples, n_samples, B);
    const int64_t nmax = sh.longest, n_fl = sh.n_fl, L = sh.L;
    const int rows = stage.rows(B);
    // rows of the dense sample block are `ns` floats apart: nmax rounded up to 4, so that every row starts on 16 bytes for any lengths (the
    // gather moves float4; a row that did not would take its scalar path -- four 4-byte reads per lane over PCIe)
    const int64_t ns = (nmax + 3) & ~(int64_t)3;
    const int64_t nb_s = align_up((int64_t)sizeof(float) * B * ns, 16);
    // the host block: [samples (not with pinned_src)] | feature offsets | feature lengths | [sample pointers | sample counts]
    const int64_t hb_s = pinned_src ? 0 : nb_s, hb_in = hb_s + 32 * (int64_t)B;
    // streams that hold input at another rate (set_wave_srcs): the resampler's row descriptors ride behind the table, and
    // resample_gather fills the dense block in place of gather_samples
    bool rs = false;
    for (int b = 0; b < B && wave_srcs_; b++) rs = rs || wave_srcs_[b].plan;
    K2_REQUIRE(!rs || pinned_src, "offline_greedy_from_samples: input at another rate is read from the streams' pinned queues only");
    const int64_t nb_rows = rs ? align_up((int64_t)sizeof(ResampleRow) * B, 16) : 0;
    // (sized for the token download as well: finish_tokens takes the same buffer and must not re-allocate it under the upload)
    char* pin = static_cast<char*>(pinned(std::max<int64_t>(hb_in + nb_rows, SearchOut::bytes_for(rows, max_tokens)) + 64));
    ResampleRow* h_rows = reinterpret_cast<ResampleRow*>(pin + hb_in);
    long long* h_off = reinterpret_cast<long long*>(pin + hb_s);
    long long* h_len = h_off + B;
    const float** h_ptr = reinterpret_cast<const float**>(h_len + B);
    long long* h_cnt = reinterpret_cast<long long*>(h_ptr + B);
    if (pinned_src) {
        for (int b = 0; b < B; b++) {
            void* dp = nullptr;   // (the device's address of the pinned array: the same value on this platform, asked for all the same)
            K2_HIP(hipHostGetDevicePointer(&dp, const_cast<float*>(samples[b]), 0));
            h_ptr[b] = static_cast<const float*>(dp);
            h_cnt[b] = n_samples[b];
            if (rs)
                h_rows[b] = resample_row(wave_srcs_[b].plan, h_ptr[b], n_samples[b], nullptr, 0, wave_srcs_[b].x0, wave_srcs_[b].k0,
                                         wave_srcs_[b].plan ? wave_count(b, n_samples[b]) : 0, b);
        }
    } else {
        auto stage = [&](int b_lo, int b_hi) {
            for (int b = b_lo; b < b_hi; b++) {
                float* row = reinterpret_cast<float*>(pin) + (size_t)b * ns;
                memcpy(row, samples[b], sizeof(float) * (size_t)n_samples[b]);
                if (n_samples[b] < ns) memset(row + n_samples[b], 0, sizeof(float) * (size_t)(ns - n_samples[b]));
            }
        };
        // 20 MB for a 32 x 10 s batch: one host thread copies it in ~2 ms (a seventh of the whole call); four do it in ~0.5 ms
        const int64_t stage_bytes = (int64_t)sizeof(float) * B * ns;
        const int helpers = stage_bytes >= (4 << 20) ? std::min(3, B - 1) : 0;
        if (helpers > 0) {
            std::vector<std::thread> th;
            const int per = (B + helpers) / (helpers + 1);
            for (int h = 1; h <= helpers; h++) th.emplace_back(stage, std::min(B, h * per), std::min(B, (h + 1) * per));
            stage(0, std::min(B, per));
            for (auto& t : th) t.join();
        } else {
            stage(0, B);
        }
    }
    for (int b = 0; b < B; b++) {
        h_off[b] = (long long)b * n_fl;
        h_len[b] = fbank_num_frames(wave_count(b, n_samples[b])) * model_->cfg().feat;
    }
    SearchOut out;
    SearchExtras ex;
    run_sized([&](const Ctx& c) {
        Arena& ar = *c.arena;
        out = SearchOut(ar, rows, max_tokens);
        char* d_in = ar.take<char>(nb_s + 32 * (int64_t)B + nb_rows);
        float* d_s = reinterpret_cast<float*>(d_in);
        long long* d_off = reinterpret_cast<long long*>(d_in + nb_s);
        long long* d_len = d_off + B;
        const float* const* d_ptr = reinterpret_cast<const float* const*>(d_len + B);
        const long long* d_cnt = reinterpret_cast<const long long*>(d_ptr + B);
        float* d_feats = ar.take<float>((int64_t)B * n_fl);
        float* d_x = ar.take<float>((int64_t)B * L);
        if (!c.dry) {
            K2_HIP(hipEventRecord(ev_[0], c.stream));
            if (pinned_src) K2_HIP(hipMemcpyAsync(d_in + nb_s, pin, (size_t)(32 * (int64_t)B + nb_rows), hipMemcpyHostToDevice, c.stream));
            else K2_HIP(hipMemcpyAsync(d_in, pin, (size_t)(nb_s + 16 * (int64_t)B), hipMemcpyHostToDevice, c.stream));
        }
        if (rs) resample_gather(c, h_rows, reinterpret_cast<const ResampleRow*>(d_in + nb_s + 32 * (int64_t)B), B, d_s, B, ns);
        else if (pinned_src) gather_samples(c, d_ptr, d_cnt, d_s, B, ns);
        fbank(c, fbank_args(d_s, nmax, ns, B, sh.frames, d_feats));
        if (!c.dry) K2_HIP(hipEventRecord(ev_[1], c.stream));
        pad_logfloor(c, d_feats, d_off, d_len, d_x, B, L);
        ex = encode_and_search(c, d_x, B, sh.T, stage, out);
    });
    finish_tokens(out, ex, tokens, ts, n_tokens);
    fill_timing(true, true);
}

int Engine::submit_samples_dev(const float* samples_dev, int64_t n_each, int B, int max_tokens) {
    K2_REQUIRE(samples_dev != nullptr, "offline_submit: bad arguments");
    return submit_impl(samples_dev, nullptr, n_each, B, max_tokens);
}
int Engine::submit_samples_host(const float* samples_host, int64_t n_each, int B, int max_tokens) {
    K2_REQUIRE(samples_host != nullptr, "offline_submit: bad arguments");
    return submit_impl(nullptr, samples_host, n_each, B, max_tokens);
}

// samples_host != nullptr: the batch's samples are still in host memory ([B, n_each] f32, ideally pinned: k2hip_host_alloc).
// The H2D copy goes on the slot's own stream, so it runs under the previous batch's encoder, and the encoder stream waits
// for it through an event -- PCIe is inside the pipeline, not in front of it.
int Engine::submit_impl(const float* samples_dev, const float* samples_host, int64_t n_each, int B, int max_tokens) {
    K2_REQUIRE(B > 0 && max_tokens > 0, "offline_submit: bad arguments");
    const OfflineShape sh = offline_shape("offline_submit", n_each);
    // slots in use: all three when every slot's search runs on the slot's own stream (the beam search), else two.  (Rounds 1 - 4 kept a
    // third form behind a switch, two whole batches concurrently on two streams: 15.15 against 13.76 ms per headline batch; removed.)
    const bool deep = beam_ > 0 && !model_->cfg().ctc;
    const int nslots = deep ? kSlots : 2;
    int ticket = -1, in_flight = 0;
    for (const auto& x : slots_) in_flight += x.busy;
    for (int k = 0; k < kSlots && ticket < 0; k++) {
        const int cand = (next_slot_ + k) % kSlots;
        if (!slots_[cand].busy && cand < nslots) ticket = cand;
    }
    if (ticket < 0 || in_flight >= nslots)
        failf(K2HIP_ERR_INVALID, "offline_submit: %d batches already in flight; wait for one first", in_flight);
    Slot& sl = slots_[ticket];
    if (!sl.stream) K2_HIP(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
    const int64_t nb = SearchOut::bytes_for(B, max_tokens);
    if (nb > sl.pin_cap) {
        if (sl.pin) K2_HIP(hipHostFree(sl.pin));
        sl.pin = nullptr;
        sl.pin_cap = 0;
        K2_HIP(hipHostMalloc(&sl.pin, (size_t)nb, hipHostMallocDefault));
        sl.pin_cap = nb;
    }
    cur_arena_ = &sl.arena;
    hipStream_t s2 = deep ? sl.stream : stream2_;
    try {
        run_sized([&](const Ctx& c) {
            Arena& ar = *c.arena;
            sl.out = SearchOut(ar, B, max_tokens);
            float* d_feats = ar.take<float>((int64_t)B * sh.n_fl);
            float* d_x = ar.take<float>((int64_t)B * sh.L);
            const float* src = samples_dev;
            if (samples_host) {
                float* d_s = ar.take<float>((int64_t)B * n_each);
                src = d_s;
                if (!c.dry) {
                    hipStream_t cs = deep ? stream2_ : sl.stream;  // deep: the shared search stream is idle -> copies
                    K2_HIP(hipMemcpyAsync(d_s, samples_host, sizeof(float) * (size_t)B * n_each, hipMemcpyHostToDevice, cs));
                    K2_HIP(hipEventRecord(sl.h2d_done, cs));
                    K2_HIP(hipStreamWaitEvent(c.stream, sl.h2d_done, 0));
                }
            }
            fbank(c, fbank_args(src, n_each, n_each, B, sh.frames, d_feats));
            pad_logfloor_dense(c, d_feats, sh.n_fl, d_x, B, sh.L);
            int Tp = 0;
            float* enc = encoder_forward(c, d_x, B, sh.T, &Tp, -1, nullptr, nullptr, nullptr);
            Ctx cd = c;
            cd.stream = s2;
            cd.instrument = false;
            cd.greedy_rec = &sl.greedy;
            sl.greedy.valid = false;
            if (!c.dry) {
                K2_HIP(hipEventRecord(sl.enc_done, c.stream));
                K2_HIP(hipStreamWaitEvent(s2, sl.enc_done, 0));
            }
            search_device(cd, enc, B, Tp, SearchStage{false, false}, sl.out);
        });
    } catch (...) {
        cur_arena_ = &arena_;
        throw;
    }
    cur_arena_ = &arena_;
    download_search(sl.out, s2, sl.pin);
    K2_HIP(hipEventRecord(sl.done, s2));
    sl.B = B;
    sl.max_tokens = max_tokens;
    sl.search_stream = s2;
    sl.busy = true;
    next_slot_ = (ticket + 1) % nslots;
    return ticket;
}

void Engine::wait_ticket(int ticket, int64_t* tokens, int32_t* ts, int32_t* n_tokens) {
    K2_REQUIRE(ticket >= 0 && ticket < kSlots && slots_[ticket].busy, "offline_wait: ticket %d is not in flight", ticket);
    K2_HIP(hipSetDevice(device_));
    Slot& sl = slots_[ticket];
    K2_HIP(hipEventSynchronize(sl.done));
    sl.busy = false;
    settle_search(sl.out, sl.search_stream, sl.greedy, sl.pin);
    SearchOut(sl.pin, sl.B, sl.max_tokens).copy_out(tokens, ts, n_tokens);
}

namespace {
struct DevBufs {  // device buffers of a tuning / test hook, freed on every way out
    std::vector<void*> p;
    template <typename T>
    T* alloc(size_t n) {
        p.push_back(nullptr);
        K2_HIP(hipMalloc(&p.back(), sizeof(T) * n));
        return static_cast<T*>(p.back());
    }
    ~DevBufs() {
        for (void* q : p) (void)hipFree(q);
    }
};
}  // namespace

// tuning hook: average time of one Linear-shaped GEMM on uniform random data under the forced configuration `cfg`; max_err
// (optional) = largest |difference| from the register-staged 64x64 kernel on the same operands
float Engine::debug_gemm(int M, int N, int K, int act, bool with_res, int iters, int cfg, float* max_err) {
    K2_HIP(hipSetDevice(device_));
    std::vector<float> h((size_t)std::max((int64_t)M * K, std::max((int64_t)N * K, (int64_t)M * N)));
    uint32_t s = 12345u;
    for (auto& v : h) { s = s * 1664525u + 1013904223u; v = ((s >> 8) * (1.0f / 8388608.0f)) - 1.0f; }
    DevBufs dev;
    float* A = dev.alloc<float>((size_t)M * K);
    float* W = dev.alloc<float>((size_t)N * K);
    float* C = dev.alloc<float>((size_t)M * N);
    float* C2 = dev.alloc<float>((size_t)M * N);
    float* Rb = dev.alloc<float>((size_t)M * N);
    float* b = dev.alloc<float>((size_t)N);
    K2_HIP(fill_blocking(W, 0, sizeof(float) * (size_t)N * K));   // (the last 7 / 3 elements below are not covered by the shifted copies)
    K2_HIP(fill_blocking(Rb, 0, sizeof(float) * (size_t)M * N));
    K2_HIP(copy_blocking(A, h.data(), sizeof(float) * (size_t)M * K, hipMemcpyHostToDevice));
    K2_HIP(copy_blocking(W, h.data() + 7, sizeof(float) * ((size_t)N * K - 7), hipMemcpyHostToDevice));
    K2_HIP(copy_blocking(Rb, h.data() + 3, sizeof(float) * ((size_t)M * N - 3), hipMemcpyHostToDevice));
    K2_HIP(copy_blocking(b, h.data() + 11, sizeof(float) * (size_t)N, hipMemcpyHostToDevice));
    Ctx c = make_ctx(false);
    c.instrument = false;
    c.stats = nullptr;
    GemmForceGuard force(cfg);
    float ms = 0;
    if (act >= 100) {  // the gated epilogue (101: value * sigmoid(gate) over all columns, 102: value * tanh(gate) over the first 2N/3,
                       // the rest passed through) against the plain GEMM + the gating done on the host
        const int mode = act - 100, gc = mode == 2 ? (2 * N / 3) / 32 * 32 : N, ldo = gc / 2 + (N - gc);
        K2_REQUIRE((mode == 1 || mode == 2) && N % 32 == 0 && gc >= 32 && max_err, "debug_gemm: gated mode needs N %% 32 == 0 and max_err");
        GemmArgs g;
        g.A = A; g.lda = K; g.W = W; g.ldw = K; g.bias = b; g.C = C; g.ldc = ldo; g.M = M; g.N = N; g.K = K; g.glu = mode; g.glu_cols = gc == N ? 0 : gc;
        gemm(c, g);
        K2_HIP(hipEventRecord(ev_[6], stream_));
        for (int i = 0; i < iters; i++) gemm(c, g);
        K2_HIP(hipEventRecord(ev_[7], stream_));
        debug_force_gemm_cfg(2 + 64);
        linear(c, A, K, W, b, C2, N, M, K, N, ACT_NONE, nullptr, 0);
        K2_HIP(hipStreamSynchronize(stream_));
        K2_HIP(hipEventElapsedTime(&ms, ev_[6], ev_[7]));
        std::vector<float> h1((size_t)M * ldo), h2((size_t)M * N);
        K2_HIP(copy_blocking(h1.data(), C, sizeof(float) * h1.size(), hipMemcpyDeviceToHost));
        K2_HIP(copy_blocking(h2.data(), C2, sizeof(float) * h2.size(), hipMemcpyDeviceToHost));
        float e = 0;
        for (int m = 0; m < M; m++)
            for (int col = 0; col < N; col++) {
                float want;
                int oc;
                if (col < gc) {
                    if (col & 16) continue;  // a gate column
                    const float v = h2[(size_t)m * N + col], gt = h2[(size_t)m * N + col + 16];
                    want = mode == 2 ? v * tanhf(gt) : v / (1.0f + expf(-gt));
                    oc = ((col >> 5) << 4) + (col & 15);
                } else {
                    want = h2[(size_t)m * N + col];
                    oc = gc / 2 + (col - gc);
                }
                const float d = fabsf(h1[(size_t)m * ldo + oc] - want);
                e = (d > e || d != d) ? (d != d ? INFINITY : d) : e;
            }
        *max_err = e;
        return ms / std::max(1, iters);
    }
    for (int i = 0; i < 3; i++) linear(c, A, K, W, b, C, N, M, K, N, act, with_res ? Rb : nullptr, N);
    K2_HIP(hipEventRecord(ev_[6], stream_));
    for (int i = 0; i < iters; i++) linear(c, A, K, W, b, C, N, M, K, N, act, with_res ? Rb : nullptr, N);
    K2_HIP(hipEventRecord(ev_[7], stream_));
    K2_HIP(hipStreamSynchronize(stream_));
    K2_HIP(hipEventElapsedTime(&ms, ev_[6], ev_[7]));
    if (max_err) {
        debug_force_gemm_cfg(2 + 64);
        linear(c, A, K, W, b, C2, N, M, K, N, act, with_res ? Rb : nullptr, N);
        K2_HIP(hipStreamSynchronize(stream_));
        std::vector<float> h1((size_t)M * N), h2((size_t)M * N);
        K2_HIP(copy_blocking(h1.data(), C, sizeof(float) * h1.size(), hipMemcpyDeviceToHost));
        K2_HIP(copy_blocking(h2.data(), C2, sizeof(float) * h2.size(), hipMemcpyDeviceToHost));
        float e = 0;
        for (size_t i = 0; i < h1.size(); i++) {
            const float d = fabsf(h1[i] - h2[i]);
            e = (d > e || d != d) ? (d != d ? INFINITY : d) : e;
        }
        *max_err = e;
    }
    return ms / iters;
}

void Engine::debug_gemm_host(const float* hA, const float* hW, const float* hb, const float* hres, float* hC, int M, int N, int K, int act,
                             int glu, int glu_cols, int cfg) {
    K2_HIP(hipSetDevice(device_));
    K2_REQUIRE(M > 0 && N > 0 && K > 0 && hA && hW && hC, "debug_gemm_host: bad arguments");
    K2_REQUIRE(glu == 0 || (N % 32 == 0 && (glu_cols == 0 || (glu_cols % 32 == 0 && glu_cols <= N))), "debug_gemm_host: gated form needs N %% 32 == 0");
    const int gc = glu ? (glu_cols ? glu_cols : N) : 0;
    const int ldo = glu ? gc / 2 + (N - gc) : N;
    DevBufs dev;
    float* A = dev.alloc<float>((size_t)M * K);
    float* W = dev.alloc<float>((size_t)N * K);
    float* C = dev.alloc<float>((size_t)M * ldo);
    float *R = nullptr, *b = nullptr;
    K2_HIP(copy_blocking(A, hA, sizeof(float) * (size_t)M * K, hipMemcpyHostToDevice));
    K2_HIP(copy_blocking(W, hW, sizeof(float) * (size_t)N * K, hipMemcpyHostToDevice));
    K2_HIP(fill_blocking(C, 0xff, sizeof(float) * (size_t)M * ldo));   // NaN pattern: an element the kernel never writes fails the comparison
    if (hb) {
        b = dev.alloc<float>((size_t)N);
        K2_HIP(copy_blocking(b, hb, sizeof(float) * (size_t)N, hipMemcpyHostToDevice));
    }
    if (hres) {
        R = dev.alloc<float>((size_t)M * ldo);
        K2_HIP(copy_blocking(R, hres, sizeof(float) * (size_t)M * ldo, hipMemcpyHostToDevice));
    }
    Ctx c = make_ctx(false);
    c.instrument = false;
    c.stats = nullptr;
    GemmArgs g;
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.bias = b; g.C = C; g.ldc = ldo; g.M = M; g.N = N; g.K = K;
    g.act = act; g.res = R; g.ldr = ldo; g.glu = glu; g.glu_cols = gc == N ? 0 : gc;
    GemmForceGuard force(cfg);
    gemm(c, g);
    K2_HIP(hipStreamSynchronize(stream_));
    K2_HIP(copy_blocking(hC, C, sizeof(float) * (size_t)M * ldo, hipMemcpyDeviceToHost));
}

// test hook: ONE launch of a launcher of kernels.h on the caller's host operands (tests/test_kernels_gpu.py, test_family_kernels_gpu.py,
// test_outer_kernels_gpu.py).  Buffer k of the call is
// uploaded into an allocation with kGuard bytes of 0xff (NaN) on either side, so a read past either end whose value reaches the result
// shows as NaN; after the launch the guards must still hold 0xff, else a write went past the buffer and the call fails naming it.
// A launcher that refuses the shape (a false return, a K2_REQUIRE) fails as K2HIP_ERR_UNSUPPORTED before anything is launched or
// downloaded.  iargs: the launcher's int arguments in its own order, a RingRef counting as (slot_stride, off); bufs: its pointer
// arguments in order, a RingRef as (pool, slots, chunks), a FullDimSegs as (src[0 .. n), lz_orig, lz_xd, lz_scale) with its ints
// (n, ld[0 .. n), col1[0 .. n), lz_Td, lz_ds, lz_Do) in front of the launcher's.  A null buffer (or 0 bytes) passes nullptr.  A float
// argument (conformer_qprep's and conformer_scores_softmax's scaling) sits among the ints as its IEEE-754 bits.
static const bool kDebugOpSet = (Engine::debug_op = &Engine::debug_op_host, true);
void Engine::debug_op_host(const char* op, const int64_t* iargs, int n_iargs, void* const* bufs, const int64_t* buf_bytes, int n_bufs,
                           uint32_t out_mask) {
    K2_HIP(hipSetDevice(device_));
    K2_REQUIRE(op && n_iargs >= 0 && n_bufs >= 0 && n_bufs <= 32 && (n_iargs == 0 || iargs) && (n_bufs == 0 || (bufs && buf_bytes)),
               "debug_op_run: bad arguments");
    constexpr int64_t kGuard = 16 * 1024;
    struct Bufs {
        hipStream_t stream;
        std::vector<char*> base;
        ~Bufs() {
            (void)hipStreamSynchronize(stream);   // (a launcher that failed after a launch: nothing is freed under a running kernel)
            for (char* p : base) (void)hipFree(p);
        }
    } d{stream_, {}};
    std::vector<void*> dev(n_bufs, nullptr);
    for (int k = 0; k < n_bufs; k++) {
        K2_REQUIRE(buf_bytes[k] >= 0 && buf_bytes[k] % 4 == 0, "debug_op_run: buffer %d has %lld bytes", k, (long long)buf_bytes[k]);
        if (!bufs[k] || buf_bytes[k] == 0) continue;
        char* p = nullptr;
        const size_t total = (size_t)(2 * kGuard + buf_bytes[k]);
        K2_HIP(hipMalloc(&p, total));
        d.base.push_back(p);
        K2_HIP(fill_blocking(p, 0xff, total));
        K2_HIP(copy_blocking(p + kGuard, bufs[k], (size_t)buf_bytes[k], hipMemcpyHostToDevice));
        dev[k] = p + kGuard;
    }
    int ni = 0, nbuf = 0;
    auto I = [&]() -> int {
        K2_REQUIRE(ni < n_iargs, "debug_op_run %s: too few int arguments (%d)", op, n_iargs);
        return (int)iargs[ni++];
    };
    auto L = [&]() -> long long {
        K2_REQUIRE(ni < n_iargs, "debug_op_run %s: too few int arguments (%d)", op, n_iargs);
        return (long long)iargs[ni++];
    };
    auto F = [&]() -> float {   // a float argument: its IEEE-754 bit pattern in the int slot
        const uint32_t u = (uint32_t)L();
        float f;
        memcpy(&f, &u, sizeof f);
        return f;
    };
    auto P = [&]() -> float* {
        K2_REQUIRE(nbuf < n_bufs, "debug_op_run %s: too few buffers (%d)", op, n_bufs);
        return static_cast<float*>(dev[nbuf++]);
    };
    auto ring = [&]() {   // (pool, slots, chunks) buffers, (slot_stride, off) ints
        RingRef r;
        r.slot_stride = L(); r.off = L();
        r.pool = P(); r.slots = reinterpret_cast<const int*>(P()); r.chunks = reinterpret_cast<const int*>(P());
        return r;
    };
    Ctx c = make_ctx(false);
    c.instrument = false;
    c.stats = nullptr;
    const std::string name = op;
    bool took = true;
    try {
        if (name == "attn_scores_softmax") {
            const int ld = I();
            float *qkp = P(), *pp = P(), *aw = P();
            const int B = I(), T = I(), Tp = I(), H = I(), qh = I(), koff0 = I(), poff0 = I();
            attn_scores_softmax(c, qkp, ld, pp, aw, B, T, Tp, H, qh, koff0, poff0);
        } else if (name == "attn_av_out") {
            float *aw = P(), *v = P(), *wout = P(), *bias = P(), *x = P();
            const int B = I(), T = I(), KL = I(), Tp = I(), H = I(), vh = I(), D = I();
            took = attn_av_out(c, aw, v, wout, bias, x, B, T, KL, Tp, H, vh, D);
        } else if (name == "attn_av_out_ring") {
            float* aw = P();
            const RingRef r = ring();
            float *newrows = P(), *wout = P(), *bias = P(), *x = P();
            const int B = I(), T = I(), KL = I(), Tp = I(), H = I(), vh = I(), D = I();
            took = attn_av_out_ring(c, aw, r, newrows, wout, bias, x, B, T, KL, Tp, H, vh, D);
        } else if (name == "attn_proj_av_out_ring") {
            float* aw = P();
            const RingRef r = ring();
            float *xin = P(), *win = P(), *bin = P(), *wout = P(), *bias = P(), *xout = P();
            const int B = I(), T = I(), KL = I(), Tp = I(), H = I(), vh = I(), D = I();
            attn_proj_av_out_ring(c, aw, r, xin, win, bin, wout, bias, xout, B, T, KL, Tp, H, vh, D);
        } else if (name == "nonlin_av_out_ring") {
            float* aw = P();
            const RingRef r = ring();
            float* hid = P();
            const int ldh = I();
            float *wout = P(), *bias = P(), *x = P();
            const int B = I(), T = I(), KL = I(), Tp = I(), Hc = I(), D = I();
            nonlin_av_out_ring(c, aw, r, hid, ldh, wout, bias, x, B, T, KL, Tp, Hc, D);
        } else if (name == "attn_stream_ring" || name == "attn_stream") {
            float* qkp = P();
            const int ld = I();
            RingRef r;
            float* kcat = nullptr;
            if (name == "attn_stream_ring") r = ring(); else kcat = P();
            float* pp = P();
            const long long* plen = reinterpret_cast<const long long*>(P());
            float* aw = P();
            const int B = I(), Tc = I(), Lc = I(), KLp = I(), H = I(), ds = I(), left50 = I();
            if (kcat) attn_stream(c, qkp, ld, kcat, pp, plen, aw, B, Tc, Lc, KLp, H, ds, left50);
            else attn_stream_ring(c, qkp, ld, r, pp, plen, aw, B, Tc, Lc, KLp, H, ds, left50);
        } else if (name == "glu_causal_conv") {
            float *x2 = P(), *pool = P();
            const long long ss = L(), off = L();
            const int* slots = reinterpret_cast<const int*>(P());
            float *wc = P(), *bc = P(), *ww = P(), *bw = P(), *sc = P(), *y = P();
            const int B = I(), Tc = I(), D = I(), K = I();
            glu_causal_conv(c, x2, pool, ss, off, slots, wc, bc, ww, bw, sc, y, B, Tc, D, K);
        } else if (name == "gemm") {
            // every int / stride field of GemmArgs in its declared order (no tuning fields, no cf_*: that form is the next op), the cfg
            // force code, res_is_C, then the float offsets of A, W, res, C, mul, byp_orig inside their buffers
            GemmArgs g;
            g.M = I(); g.N = I(); g.K = I();
            g.lda = I(); g.ldw = I(); g.ldc = I(); g.ldr = I();
            g.act = I(); g.act_cols = I(); g.w_kn = I();
            g.nb0 = I(); g.nb1 = I();
            g.sA0 = L(); g.sA1 = L(); g.sW0 = L(); g.sW1 = L(); g.sC0 = L(); g.sC1 = L(); g.sR0 = L(); g.sR1 = L();
            g.sBias0 = L();
            g.cv_Fout = I(); g.cv_Tout = I(); g.cv_Tin = I(); g.cv_Fin = I(); g.cv_C = I(); g.cv_st = I(); g.cv_sf = I();
            g.seg_len = I(); g.seg_stride = I();
            g.res_div = I(); g.act_after_res = I();
            g.glu = I(); g.glu_cols = I();
            g.ldm = I(); g.sM0 = L(); g.sM1 = L();
            g.ld_orig = I();
            const int cfg = I(), res_is_C = I();
            const long long oA = L(), oW = L(), oR = L(), oC = L(), oM = L(), oO = L();
            float *A = P(), *W = P(), *bias = P(), *res = P(), *C = P();
            const int* skip = reinterpret_cast<const int*>(P());
            float *mul = P(), *orig = P(), *scale = P();
            int* plan_out = reinterpret_cast<int*>(P());
            K2_REQUIRE(A && W && C && plan_out && buf_bytes[n_bufs - 1] >= 20, "debug_op_run gemm: A, W, C and a plan buffer of 5 ints are needed");
            K2_REQUIRE(!(res_is_C && res), "debug_op_run gemm: res_is_C takes no res buffer");
            K2_REQUIRE(oA >= 0 && oW >= 0 && oR >= 0 && oC >= 0 && oM >= 0 && oO >= 0, "debug_op_run gemm: negative offset");
            if (res_is_C) res = C;
            g.A = A + oA; g.W = W + oW; g.bias = bias; g.res = res ? res + oR : nullptr; g.C = C + oC;
            g.skip_if_zero = skip;
            g.mul = mul ? mul + oM : nullptr;
            g.byp_orig = orig ? orig + oO : nullptr; g.byp_scale = scale;
            GemmForceGuard force(cfg);
            const GemmPlan pl = plan_gemm(g, gemm_force());
            const int rep[5] = {(int)pl.family, pl.idx, pl.BM, pl.BN, pl.mode};
            K2_HIP(copy_blocking(plan_out, rep, sizeof rep, hipMemcpyHostToDevice));
            gemm(c, g);
        } else if (name == "gemm_glu_causal_conv") {
            float *x = P(), *wg = P(), *bg = P(), *pool = P();
            const long long ss = L(), off = L();
            const int* slots = reinterpret_cast<const int*>(P());
            float *wc = P(), *bc = P(), *ww = P(), *bw = P(), *sc = P(), *y = P();
            const int B = I(), Tc = I(), D = I(), K = I();
            int* entry_out = reinterpret_cast<int*>(P());
            K2_REQUIRE(entry_out && buf_bytes[n_bufs - 1] >= 4, "debug_op_run gemm_glu_causal_conv: an entry buffer of 1 int is needed");
            const int entry = glu_conv_ring_entry(B, Tc, D, K);
            K2_HIP(copy_blocking(entry_out, &entry, sizeof entry, hipMemcpyHostToDevice));
            took = gemm_glu_causal_conv(c, x, wg, bg, pool, ss, off, slots, wc, bc, ww, bw, sc, y, B, Tc, D, K);
        } else if (name == "gemm_glu_dwconv1d") {
            // the offline conv module's in_proj + GLU + depthwise conv + SwooshR as the layer body runs it for the shape: the fused launch
            // where glu_dwconv_pipe_entry has one, else the GLU GEMM + dwconv1d_swoosh (M >= 256), else linear + glu_dwconv1d_swoosh
            const int wg_k = nbuf + 1, bg_k = nbuf + 2;   // (the host copies of wg and bg, for the plain in_proj below)
            float *x = P(), *wg = P(), *bg = P(), *wd = P(), *bd = P(), *y = P();
            const int B = I(), T = I(), D = I(), K = I();
            int* entry_out = reinterpret_cast<int*>(P());
            K2_REQUIRE(x && wg && bg && wd && bd && y && entry_out && buf_bytes[n_bufs - 1] >= 4, "debug_op_run gemm_glu_dwconv1d: six operands and an entry buffer of 1 int are needed");
            K2_REQUIRE(B >= 1 && T >= 1 && D >= 16 && D % 16 == 0 && K >= 1, "debug_op_run gemm_glu_dwconv1d: B %d T %d D %d K %d", B, T, D, K);
            const int M = B * T;
            const int entry = glu_dwconv_pipe_entry(B, T, D, K, false);
            K2_HIP(copy_blocking(entry_out, &entry, sizeof entry, hipMemcpyHostToDevice));
            auto scratch = [&](size_t floats) {
                char* p = nullptr;
                K2_HIP(hipMalloc(&p, floats * sizeof(float)));
                d.base.push_back(p);
                return reinterpret_cast<float*>(p);
            };
            const bool fused = gemm_glu_dwconv1d(c, x, wg, bg, wd, bd, y, B, T, D, K);
            if (fused) {
                // (entry >= 0: the one launch has written y)
            } else if (M >= 256 && !tunables().no_glu_epilogue) {
                float* hid = scratch((size_t)M * D);
                GemmArgs g;
                g.A = x; g.lda = D; g.W = wg; g.ldw = D; g.bias = bg;
                g.C = hid; g.ldc = D; g.M = M; g.N = 2 * D; g.K = D; g.glu = 1;
                gemm(c, g);
                dwconv1d_swoosh(c, hid, wd, bd, y, B, T, D, K);
            } else {   // the plain in_proj: the "#glu" rows back in (value rows | gate rows) order (model.cpp interleaves them at load)
                const float *hw = static_cast<const float*>(bufs[wg_k]), *hb = static_cast<const float*>(bufs[bg_k]);
                std::vector<float> vw((size_t)2 * D * D), vb((size_t)2 * D);
                for (int ch = 0; ch < D; ch++) {
                    const int rv = 32 * (ch / 16) + ch % 16, rg = rv + 16;
                    memcpy(&vw[(size_t)ch * D], &hw[(size_t)rv * D], sizeof(float) * D);
                    memcpy(&vw[(size_t)(D + ch) * D], &hw[(size_t)rg * D], sizeof(float) * D);
                    vb[ch] = hb[rv];
                    vb[D + ch] = hb[rg];
                }
                float *wp = scratch(vw.size()), *bp = scratch(vb.size()), *hid = scratch((size_t)M * 2 * D);
                K2_HIP(copy_blocking(wp, vw.data(), vw.size() * sizeof(float), hipMemcpyHostToDevice));
                K2_HIP(copy_blocking(bp, vb.data(), vb.size() * sizeof(float), hipMemcpyHostToDevice));
                linear(c, x, D, wp, bp, hid, 2 * D, M, D, 2 * D);
                glu_dwconv1d_swoosh(c, hid, wd, bd, y, B, T, D, K);
            }
        } else if (name == "biasnorm") {
            float *x = P(), *bias = P(), *ls = P(), *y = P();
            const int M = I(), D = I();
            biasnorm(c, x, bias, ls, y, M, D);
        } else if (name == "bypass") {
            float *orig = P(), *x = P(), *scale = P(), *y = P();
            const int M = I(), D = I();
            bypass(c, orig, x, scale, y, M, D);
        } else if (name == "biasnorm_bypass") {
            float *x = P(), *orig = P(), *nb = P(), *ls = P(), *scale = P(), *y = P();
            const int M = I(), D = I();
            biasnorm_bypass(c, x, orig, nb, ls, scale, y, M, D);
        } else if (name == "biasnorm_bypass_downsample") {
            float *x = P(), *orig = P(), *nb = P(), *ls = P(), *scale = P(), *y = P(), *bias2 = P(), *xd2 = P();
            const int B = I(), T = I(), D = I(), ds2 = I(), D2 = I();
            biasnorm_bypass_downsample(c, x, orig, nb, ls, scale, y, bias2, xd2, B, T, D, ds2, D2);
        } else if (name == "downsample") {
            float *x = P(), *bias = P(), *y = P();
            const int B = I(), T = I(), D = I(), ds = I(), Din = I();
            downsample(c, x, bias, y, B, T, D, ds, Din);
        } else if (name == "downsample_full") {
            FullDimSegs s;
            s.n = I();
            K2_REQUIRE(s.n >= 1 && s.n <= 8, "debug_op_run downsample_full: %d segments", s.n);
            for (int k = 0; k < s.n; k++) s.ld[k] = I();
            for (int k = 0; k < s.n; k++) s.col1[k] = I();
            s.lz_Td = I(); s.lz_ds = I(); s.lz_Do = I();
            for (int k = 0; k < s.n; k++) s.src[k] = P();
            s.lz_orig = P(); s.lz_xd = P(); s.lz_scale = P();
            float *bias = P(), *y = P();
            const int B = I(), T = I(), D = I(), ds = I();
            downsample_full(c, s, bias, y, B, T, D, ds);
        } else if (name == "upsample_combine") {
            float *orig = P(), *xd = P(), *scale = P(), *y = P();
            const int B = I(), T = I(), Td = I(), D = I(), ds = I(), Dorig = I();
            upsample_combine(c, orig, xd, scale, y, B, T, Td, D, ds, Dorig);
        } else if (name == "upsample_combine_downsample") {
            float *orig = P(), *xd = P(), *scale = P(), *y = P(), *bias2 = P(), *xd2 = P();
            const int B = I(), T = I(), Td = I(), D = I(), ds = I(), Dorig = I(), D2 = I(), ds2 = I();
            upsample_combine_downsample(c, orig, xd, scale, y, bias2, xd2, B, T, Td, D, ds, Dorig, D2, ds2);
        } else if (name == "glu_dwconv1d_swoosh" || name == "glu_dwconv1d_dswish" || name == "dwconv1d_swoosh") {
            float *x = P(), *w = P(), *b = P(), *y = P();
            const int B = I(), T = I(), D = I(), K = I();
            if (name == "glu_dwconv1d_swoosh") glu_dwconv1d_swoosh(c, x, w, b, y, B, T, D, K);
            else if (name == "glu_dwconv1d_dswish") glu_dwconv1d_dswish(c, x, w, b, y, B, T, D, K);
            else dwconv1d_swoosh(c, x, w, b, y, B, T, D, K);
        } else if (name == "dwconv7x7") {
            float *x = P(), *w = P(), *b = P(), *y = P();
            const int B = I(), Tin = I(), Tout = I(), tpad = I(), F = I(), C = I();
            dwconv7x7(c, x, w, b, y, B, Tin, Tout, tpad, F, C);
        // ---- offline / streaming Conformer (conformer.hip); a float argument travels in the int slot as its IEEE-754 bits
        } else if (name == "conformer_qprep") {
            float *qkv = P(), *bu = P(), *bv = P(), *qu = P(), *qv = P();
            const int M = I(), D = I();
            const float scaling = F();
            const int ldq = I();
            conformer_qprep(c, qkv, bu, bv, qu, qv, M, D, scaling, ldq);
        } else if (name == "conformer_scores_softmax") {
            float *qu = P(), *qv = P(), *kmat = P();
            const int ldk = I();
            float *pp = P(), *aw = P();
            const int B = I(), H = I(), T = I(), Tp = I(), D = I(), ldq = I();
            float *bu = P(), *bv = P();
            const float scaling = F();
            took = conformer_scores_softmax(c, qu, qv, kmat, ldk, pp, aw, B, H, T, Tp, D, ldq, bu, bv, scaling);
        } else if (name == "conformer_softmax_shift") {
            float *ac = P(), *bd = P();
            const int Z = I(), T = I(), Tp = I(), NPp = I();
            conformer_softmax_shift(c, ac, bd, Z, T, Tp, NPp);
        } else if (name == "conformer_softmax_shift_stream") {
            float *ac = P(), *bd = P();
            const long long* plen = reinterpret_cast<const long long*>(P());
            const int B = I(), H = I(), Tc = I(), left = I(), KLp = I(), NPp = I();
            conformer_softmax_shift_stream(c, ac, bd, plen, B, H, Tc, left, KLp, NPp);
        } else if (name == "slice_rows") {
            float *in = P(), *out = P();
            const int B = I(), Tin = I(), row0 = I(), Tout = I(), D = I();
            slice_rows(c, in, out, B, Tin, row0, Tout, D);
        } else if (name == "dwconv_valid_dswish") {
            float *cat = P(), *w = P(), *bias = P(), *y = P();
            const int B = I(), Tc = I(), D = I(), K = I();
            dwconv_valid_dswish(c, cat, w, bias, y, B, Tc, D, K);
        // ---- Zipformer v1 (zipformer1.hip)
        } else if (name == "z1_pool") {
            float *x = P(), *pool = P();
            const long long ss = L(), avg_off = L(), len_off = L();
            const int* slots = reinterpret_cast<const int*>(P());
            float* out = P();
            const int B = I(), Tc = I(), D = I();
            z1_pool(c, x, pool, ss, avg_off, len_off, slots, out, B, Tc, D);
        } else if (name == "z1_attn") {
            float* qkvp = P();
            const int ld = I();
            float *kcat = P(), *pp = P(), *aw = P();
            const int B = I(), Tc = I(), Lc = I(), KLp = I(), H = I(), A = I();
            z1_attn(c, qkvp, ld, kcat, pp, aw, B, Tc, Lc, KLp, H, A);
        } else if (name == "z1_glu_conv") {
            float *x2 = P(), *pool = P();
            const long long ss = L(), off = L();
            const int* slots = reinterpret_cast<const int*>(P());
            float *w = P(), *bias = P(), *y = P();
            const int B = I(), Tc = I(), D = I(), K = I();
            z1_glu_conv(c, x2, pool, ss, off, slots, w, bias, y, B, Tc, D, K);
        } else if (name == "z1_norm_bypass") {
            float *x = P(), *orig = P(), *le = P(), *bs = P(), *y = P();
            const int M = I(), D = I();
            z1_norm_bypass(c, x, orig, le, bs, y, M, D);
        } else if (name == "z1_attn_downsample") {
            float *x = P(), *query = P(), *y = P();
            const int B = I(), T = I(), Din = I(), ldy = I(), ds = I();
            z1_attn_downsample(c, x, query, y, B, T, Din, ldy, ds);
        } else if (name == "z1_mean") {
            float *x = P(), *mean = P();
            const int B = I(), T = I(), D = I();
            z1_mean(c, x, mean, B, T, D);
        } else if (name == "z1_add_bcast") {
            float *x = P(), *v = P();
            const int B = I(), T = I(), D = I();
            z1_add_bcast(c, x, v, B, T, D);
        } else if (name == "z1_group_rows") {
            float *x = P(), *grp = P();
            const int B = I(), T = I(), Din = I(), ds = I();
            z1_group_rows(c, x, grp, B, T, Din, ds);
        } else if (name == "z1_combine") {
            float* s1 = P();
            const int d1 = I();
            float* s2 = P();
            const int d2 = I();
            float *w1 = P(), *ub = P();
            const int ds = I(), B = I(), T = I(), Td = I();
            float* y = P();
            z1_combine(c, s1, d1, s2, d2, w1, ub, ds, B, T, Td, y);
        // ---- LSTM transducer (lstm.hip) and the elementwise.hip kernels only these families use
        } else if (name == "lstm_cell") {
            float* gx = P();
            const long long ldgx = L();
            float* gh = P();
            const int ldgh = I();
            float *cc = P(), *hf = P();
            const int B = I(), Hh = I();
            lstm_cell(c, gx, ldgx, gh, ldgh, cc, hf, B, Hh);
        } else if (name == "lstm_cell_rows") {
            float *gates = P(), *cc = P(), *hf = P();
            const int rows = I(), Hh = I();
            lstm_cell_rows(c, gates, cc, hf, rows, Hh);
        } else if (name == "lstm_add_frame") {
            float* Y = P();
            const long long SY = L();
            float* hp = P();
            const long long pstride = L();
            const int S = I();
            float *h = P(), *x1 = P();
            const int n = I(), B = I(), T = I(), D = I(), lo = I(), s = I();
            lstm_add_frame(c, Y, SY, hp, pstride, S, h, x1, n, B, T, D, lo, s);
        } else if (name == "lstm_norm_frame") {
            float *x1 = P(), *fp = P();
            const long long pstride = L();
            const int S = I();
            float *b2 = P(), *eps = P();
            const long long lstride = L();
            float* Y = P();
            const long long SY = L();
            const int n = I(), B = I(), T = I(), D = I(), lo = I(), s = I();
            lstm_norm_frame(c, x1, fp, pstride, S, b2, eps, lstride, Y, SY, n, B, T, D, lo, s);
        } else if (name == "add_inplace") {
            float *a = P(), *b = P();
            const long long n = L();
            add_inplace(c, a, b, n);
        } else if (name == "gather_rows" || name == "scatter_rows") {
            float* pool = P();
            const long long ss = L(), off = L();
            const int* slots = reinterpret_cast<const int*>(P());
            float* io = P();
            if (name == "gather_rows") {
                const int B = I(), width = I();
                gather_rows(c, pool, ss, off, slots, io, B, width);
            } else {
                const int ldin = I(), B = I(), width = I();
                scatter_rows(c, pool, ss, off, slots, io, ldin, B, width);
            }
        } else if (name == "greedy_screen_counts") {
            // no launch: the model's two counters (rounds the f16 screen decided, rounds that ran the f32 passes) into bufs[0]
            float* out = P();
            K2_REQUIRE(out && buf_bytes[0] >= 16, "debug_op_run greedy_screen_counts: a buffer of 2 int64 is needed");
            K2_HIP(hipStreamSynchronize(stream_));
            K2_HIP(copy_blocking(out, d_screen_counts_, 2 * sizeof(unsigned long long), hipMemcpyDeviceToDevice));
            out_mask |= 1u;
        } else if (name == "lattice_logprobs" || name == "lattice_dp") {
            // lattice_logprobs: bufs enc [B][Tp][J], n_frames [B] int32 (or null), ids int64 back to back, lens [B] int32, stay, emit (out:
            //   every stream's plane [T_b][U_b + 1], back to back); ints B, Tp
            // lattice_dp: bufs n_frames, lens, stay, emit (in), timestamps [B][max_tokens] int32, token_log_probs [B][max_tokens],
            //   scores [B][2] = (total, best) (out); ints B, Tp, max_tokens
            const bool cells = name == "lattice_logprobs";
            K2_REQUIRE(n_bufs == (cells ? 6 : 7), "debug_op_run %s: %d buffers", op, n_bufs);
            const int k_enc = cells ? 0 : -1, k_nf = cells ? 1 : 0, k_ids = cells ? 2 : -1, k_lens = cells ? 3 : 1, k_stay = cells ? 4 : 2,
                      k_emit = k_stay + 1, k_ts = 4, k_lp = 5, k_sc = 6;
            for (int k = 0; k < n_bufs; k++) P();
            const int B = I(), Tp = I(), max_tokens = cells ? INT_MAX : I();
            K2_REQUIRE(B > 0 && Tp > 0 && max_tokens > 0, "debug_op_run %s: bad shape", op);
            K2_REQUIRE(bufs[k_lens] && buf_bytes[k_lens] >= 4 * (int64_t)B && (!bufs[k_nf] || buf_bytes[k_nf] >= 4 * (int64_t)B),
                       "debug_op_run %s: lens / n_frames are too short", op);
            const int32_t* lens = static_cast<const int32_t*>(bufs[k_lens]);
            const int32_t* nf = static_cast<const int32_t*>(bufs[k_nf]);
            int64_t n_ids = 0;
            for (int b = 0; b < B; b++) n_ids += std::max(lens[b], 0);
            std::vector<int64_t> fill;   // (lattice_dp reads no targets: any id the check accepts)
            const int64_t* ids = nullptr;
            if (cells) {
                K2_REQUIRE(n_ids == 0 || (bufs[k_ids] && buf_bytes[k_ids] >= 8 * n_ids), "debug_op_run %s: ids are too short", op);
                ids = static_cast<const int64_t*>(bufs[k_ids]);
            } else {
                fill.assign((size_t)n_ids + 1, std::min(3, model_->cfg().V - 1));
                ids = fill.data();
            }
            const AlignPlan p = align_plan(B, Tp, nf, ids, lens, max_tokens);
            K2_REQUIRE(dev[k_stay] && dev[k_emit] && buf_bytes[k_stay] >= 4 * p.plane_floats && buf_bytes[k_emit] >= 4 * p.plane_floats,
                       "debug_op_run %s: the planes need %lld floats each", op, p.plane_floats);
            if (cells) K2_REQUIRE(dev[k_enc] && buf_bytes[k_enc] >= 4 * (int64_t)B * Tp * model_->cfg().J, "debug_op_run %s: enc is too short", op);
            else
                K2_REQUIRE(dev[k_ts] && dev[k_lp] && dev[k_sc] && buf_bytes[k_ts] >= 4 * (int64_t)B * max_tokens &&
                               buf_bytes[k_lp] >= 4 * (int64_t)B * max_tokens && buf_bytes[k_sc] >= 8 * (int64_t)B,
                           "debug_op_run %s: the result buffers are too short", op);
            SearchOut out;
            SearchExtras ex;
            run_sized([&](const Ctx& cc) {
                out = SearchOut(*cc.arena, B, cells ? 1 : max_tokens);
                ex = align_device(cc, cells ? static_cast<const float*>(dev[k_enc]) : nullptr, Tp, p, out, static_cast<float*>(dev[k_stay]),
                                  static_cast<float*>(dev[k_emit]), cells, !cells);
            });
            K2_HIP(hipStreamSynchronize(stream_));
            if (!cells) {
                K2_HIP(copy_blocking(dev[k_ts], out.timestamps(), 4 * (size_t)B * max_tokens, hipMemcpyDeviceToDevice));
                K2_HIP(copy_blocking(dev[k_lp], ex.align_lp, 4 * (size_t)B * max_tokens, hipMemcpyDeviceToDevice));
                K2_HIP(copy_blocking(dev[k_sc], ex.align_scores, 8 * (size_t)B, hipMemcpyDeviceToDevice));
            }
        } else if (name == "trie_logprobs") {
            // bufs enc [B][Tp][J], n_frames [B] int32 (or null), keyword ids int64 back to back, lens [P] int32, thresholds [P], stay, emit
            //   (out: every stream's plane [T_b][S], back to back; all streams on the one graph); ints B, Tp, P
            K2_REQUIRE(n_bufs == 7, "debug_op_run %s: %d buffers", op, n_bufs);
            for (int k = 0; k < n_bufs; k++) P();
            const int B = I(), Tp = I(), NP = I();
            K2_REQUIRE(B > 0 && Tp > 0 && NP >= 0, "debug_op_run %s: bad shape", op);
            K2_REQUIRE((!bufs[1] || buf_bytes[1] >= 4 * (int64_t)B) && (NP == 0 || (bufs[3] && buf_bytes[3] >= 4 * (int64_t)NP && bufs[4] &&
                                                                                    buf_bytes[4] >= 4 * (int64_t)NP)),
                       "debug_op_run %s: n_frames / lens / thresholds are too short", op);
            const int32_t* lens = static_cast<const int32_t*>(bufs[3]);
            int64_t n_ids = 0;
            for (int k = 0; k < NP; k++) n_ids += std::max(lens[k], 0);
            K2_REQUIRE(n_ids == 0 || (bufs[2] && buf_bytes[2] >= 8 * n_ids), "debug_op_run %s: ids are too short", op);
            const KeywordGraph g(static_cast<const int64_t*>(bufs[2]), lens, static_cast<const float*>(bufs[4]), NP, model_->cfg().V);
            const int S = g.num_states();
            KwsGraphDev gd;
            char* res = static_cast<char*>(kws_graph_upload(g, &gd));
            d.base.push_back(res);
            std::vector<float> a0((size_t)S);
            std::vector<int32_t> s0((size_t)S);
            kws_fresh_state(S, a0.data(), s0.data());
            const int32_t* nf = static_cast<const int32_t*>(bufs[1]);
            std::vector<KwsIO> io((size_t)B);
            for (int b = 0; b < B; b++) io[(size_t)b] = KwsIO{&gd, nf ? nf[b] : Tp, a0.data(), s0.data()};
            const KwsPlan p = kws_plan(B, Tp, io.data(), false);
            K2_REQUIRE(dev[0] && buf_bytes[0] >= 4 * (int64_t)B * Tp * model_->cfg().J, "debug_op_run %s: enc is too short", op);
            K2_REQUIRE(dev[5] && dev[6] && buf_bytes[5] >= 4 * p.plane_floats && buf_bytes[6] >= 4 * p.plane_floats,
                       "debug_op_run %s: the planes need %lld floats each", op, p.plane_floats);
            run_sized([&](const Ctx& cc) {
                const SearchOut out(*cc.arena, B, std::max(p.max_T, 1));
                kws_device(cc, static_cast<const float*>(dev[0]), Tp, p, out, static_cast<float*>(dev[5]), static_cast<float*>(dev[6]), true, false);
            });
            K2_HIP(hipStreamSynchronize(stream_));
        } else if (name == "trie_dp") {
            // bufs n_frames [B] int32 (or null), parent, depth, kw [S] int32, bar [S], stay, emit (in: every stream's plane [T_b][S], back to
            //   back), a [B][S], start [B][S] int32 (in / out: the carried blocks), ev_keyword [B][Tp] int64, ev_start, ev_end [B][Tp] int32,
            //   ev_sum [B][Tp], n_events [B] int32 (out); ints B, Tp, S.  All streams walk the one trie; bar is taken as given.
            K2_REQUIRE(n_bufs == 14, "debug_op_run %s: %d buffers", op, n_bufs);
            for (int k = 0; k < n_bufs; k++) P();
            const int B = I(), Tp = I(), S = I();
            K2_REQUIRE(B > 0 && Tp > 0 && S >= 1 && S <= kKwsMaxStates, "debug_op_run %s: bad shape", op);
            K2_REQUIRE(!bufs[0] || buf_bytes[0] >= 4 * (int64_t)B, "debug_op_run %s: n_frames is too short", op);
            for (int k = 1; k <= 4; k++) K2_REQUIRE(dev[k] && buf_bytes[k] >= 4 * (int64_t)S, "debug_op_run %s: the trie tables are too short", op);
            const int32_t* par = static_cast<const int32_t*>(bufs[1]);
            for (int s2 = 1; s2 < S; s2++) K2_REQUIRE(par[s2] >= 0 && par[s2] < s2, "debug_op_run %s: parent(%d) = %d", op, s2, par[s2]);
            K2_REQUIRE(dev[7] && dev[8] && buf_bytes[7] >= 4 * (int64_t)B * S && buf_bytes[8] >= 4 * (int64_t)B * S,
                       "debug_op_run %s: the carried blocks are too short", op);
            KwsGraphDev gd;
            gd.dec = static_cast<const float*>(dev[1]);   // (not read: the arcs are the caller's planes)
            gd.parent = static_cast<const int*>(dev[1]); gd.depth = static_cast<const int*>(dev[2]); gd.kw = static_cast<const int*>(dev[3]);
            gd.bar = static_cast<const float*>(dev[4]);
            gd.S = S;
            const int32_t* nf = static_cast<const int32_t*>(bufs[0]);
            std::vector<KwsIO> io((size_t)B);
            for (int b = 0; b < B; b++)
                io[(size_t)b] = KwsIO{&gd, nf ? nf[b] : Tp, static_cast<const float*>(bufs[7]) + (size_t)b * S, static_cast<const int32_t*>(bufs[8]) + (size_t)b * S};
            const KwsPlan p = kws_plan(B, Tp, io.data(), false);
            K2_REQUIRE(dev[5] && dev[6] && buf_bytes[5] >= 4 * p.plane_floats && buf_bytes[6] >= 4 * p.plane_floats,
                       "debug_op_run %s: the planes need %lld floats each", op, p.plane_floats);
            const int64_t ne = (int64_t)B * Tp;
            K2_REQUIRE(dev[9] && dev[10] && dev[11] && dev[12] && dev[13] && buf_bytes[9] >= 8 * ne && buf_bytes[10] >= 4 * ne && buf_bytes[11] >= 4 * ne &&
                           buf_bytes[12] >= 4 * ne && buf_bytes[13] >= 4 * (int64_t)B,
                       "debug_op_run %s: the event buffers are too short", op);
            SearchOut out;
            SearchExtras ex;
            run_sized([&](const Ctx& cc) {
                out = SearchOut(*cc.arena, B, Tp);
                ex = kws_device(cc, nullptr, Tp, p, out, static_cast<float*>(dev[5]), static_cast<float*>(dev[6]), false, true);
            });
            K2_HIP(hipStreamSynchronize(stream_));
            K2_HIP(copy_blocking(dev[7], ex.kws_a, 4 * (size_t)B * S, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[8], ex.kws_st, 4 * (size_t)B * S, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[9], out.tokens(), 8 * (size_t)ne, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[10], ex.kws_start, 4 * (size_t)ne, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[11], out.timestamps(), 4 * (size_t)ne, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[12], ex.kws_sum, 4 * (size_t)ne, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[13], out.counts(), 4 * (size_t)B, hipMemcpyDeviceToDevice));
        } else if (name == "ctc_trie_dp") {
            // bufs log_probs [B][Tp][V], n_frames [B] int32 (or null), graph_of [B] int32 (or null = graph 0), the G graphs' tables back to
            //   back, each [parent | tok | depth | kw | bar | rc] x [S_g] (bar as given), n_states [G] int32, v, st (in / out: the carried
            //   blocks [2][S] of every stream, back to back), ev_keyword [B][Tp] int64, ev_start, ev_end [B][Tp] int32, ev_sum [B][Tp],
            //   n_events [B] int32 (out); ints B, Tp, G, V (the log-probs' width: any, not the model's)
            K2_REQUIRE(n_bufs == 12, "debug_op_run %s: %d buffers", op, n_bufs);
            for (int k = 0; k < n_bufs; k++) P();
            const int B = I(), Tp = I(), G = I(), V = I();
            K2_REQUIRE(B > 0 && Tp > 0 && G > 0 && V >= 2, "debug_op_run %s: bad shape", op);
            K2_REQUIRE((!bufs[1] || buf_bytes[1] >= 4 * (int64_t)B) && (!bufs[2] || buf_bytes[2] >= 4 * (int64_t)B) && bufs[4] && buf_bytes[4] >= 4 * (int64_t)G,
                       "debug_op_run %s: n_frames / graph_of / n_states are too short", op);
            K2_REQUIRE(dev[0] && buf_bytes[0] >= 4 * (int64_t)B * Tp * V, "debug_op_run %s: log_probs is too short", op);
            const int32_t *nf = static_cast<const int32_t*>(bufs[1]), *gof = static_cast<const int32_t*>(bufs[2]), *ns = static_cast<const int32_t*>(bufs[4]);
            std::vector<CtcKwsGraph> graphs((size_t)G);
            int64_t words = 0;
            for (int g = 0; g < G; g++) {
                K2_REQUIRE(ns[g] >= 1 && ns[g] <= kKwsMaxStates, "debug_op_run %s: graph %d has %d states", op, g, ns[g]);
                words += 6 * (int64_t)ns[g];
            }
            K2_REQUIRE(bufs[3] && buf_bytes[3] >= 4 * words, "debug_op_run %s: the tables are too short", op);
            const int32_t* tab = static_cast<const int32_t*>(bufs[3]);
            for (int g = 0; g < G; g++) {
                const int S = ns[g];
                graphs[(size_t)g] = CtcKwsGraph{tab, tab + S, tab + 2 * S, tab + 3 * S, reinterpret_cast<const float*>(tab + 4 * S), tab + 5 * S, S};
                tab += 6 * S;
            }
            std::vector<CtcKwsIO> io((size_t)B);
            int64_t cells = 0;
            for (int b = 0; b < B; b++) {
                const int g = gof ? gof[b] : 0;
                K2_REQUIRE(g >= 0 && g < G, "debug_op_run %s: stream %d names graph %d", op, b, g);
                cells += 2 * (int64_t)graphs[(size_t)g].S;
            }
            K2_REQUIRE(bufs[5] && bufs[6] && buf_bytes[5] >= 4 * cells && buf_bytes[6] >= 4 * cells, "debug_op_run %s: the carried blocks are too short", op);
            cells = 0;
            for (int b = 0; b < B; b++) {
                const CtcKwsGraph* g = &graphs[(size_t)(gof ? gof[b] : 0)];
                io[(size_t)b] = CtcKwsIO{g, nf ? nf[b] : Tp, static_cast<const float*>(bufs[5]) + cells, static_cast<const int32_t*>(bufs[6]) + cells};
                cells += 2 * (int64_t)g->S;
            }
            const CtcKwsPlan p = ctc_kws_plan(B, Tp, io.data(), false, V);
            const int64_t ne = (int64_t)B * Tp;
            K2_REQUIRE(dev[7] && dev[8] && dev[9] && dev[10] && dev[11] && buf_bytes[7] >= 8 * ne && buf_bytes[8] >= 4 * ne && buf_bytes[9] >= 4 * ne &&
                           buf_bytes[10] >= 4 * ne && buf_bytes[11] >= 4 * (int64_t)B,
                       "debug_op_run %s: the event buffers are too short", op);
            SearchOut out;
            SearchExtras ex;
            run_sized([&](const Ctx& cc) {
                out = SearchOut(*cc.arena, B, Tp);
                ex = ctc_kws_device(cc, static_cast<const float*>(dev[0]), Tp, p, out);
            });
            K2_HIP(hipStreamSynchronize(stream_));
            K2_HIP(copy_blocking(dev[5], ex.kws_a, 4 * (size_t)cells, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[6], ex.kws_st, 4 * (size_t)cells, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[7], out.tokens(), 8 * (size_t)ne, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[8], ex.kws_start, 4 * (size_t)ne, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[9], out.timestamps(), 4 * (size_t)ne, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[10], ex.kws_sum, 4 * (size_t)ne, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[11], out.counts(), 4 * (size_t)B, hipMemcpyDeviceToDevice));
        } else if (name == "ctc_lattice") {
            // bufs log_probs [R][Tp][V], n_frames [R] int32 (or null), stream_of [H] int32 (or null), ids int64 back to back, lens [H] int32,
            //   timestamps, end_frames [H][max_tokens] int32, token_log_probs [H][max_tokens], scores [H][2] = (total, best) (out);
            //   ints R, Tp, H, max_tokens
            K2_REQUIRE(n_bufs == 9, "debug_op_run %s: %d buffers", op, n_bufs);
            for (int k = 0; k < n_bufs; k++) P();
            const int R = I(), Tp = I(), H = I(), max_tokens = I();
            K2_REQUIRE(R > 0 && Tp > 0 && H > 0 && max_tokens > 0, "debug_op_run %s: bad shape", op);
            K2_REQUIRE(bufs[4] && buf_bytes[4] >= 4 * (int64_t)H && (!bufs[1] || buf_bytes[1] >= 4 * (int64_t)R) && (!bufs[2] || buf_bytes[2] >= 4 * (int64_t)H),
                       "debug_op_run %s: lens / n_frames / stream_of are too short", op);
            const int32_t* lens = static_cast<const int32_t*>(bufs[4]);
            int64_t n_ids = 0;
            for (int h = 0; h < H; h++) n_ids += std::max(lens[h], 0);
            K2_REQUIRE(n_ids == 0 || (bufs[3] && buf_bytes[3] >= 8 * n_ids), "debug_op_run %s: ids are too short", op);
            const CtcAlignPlan p = ctc_align_plan(R, Tp, static_cast<const int32_t*>(bufs[1]), H, static_cast<const int32_t*>(bufs[2]),
                                                  static_cast<const int64_t*>(bufs[3]), lens, max_tokens);
            K2_REQUIRE(dev[0] && buf_bytes[0] >= 4 * (int64_t)R * Tp * model_->cfg().V, "debug_op_run %s: log_probs is too short", op);
            K2_REQUIRE(dev[5] && dev[6] && dev[7] && dev[8] && buf_bytes[5] >= 4 * (int64_t)H * max_tokens && buf_bytes[6] >= 4 * (int64_t)H * max_tokens &&
                           buf_bytes[7] >= 4 * (int64_t)H * max_tokens && buf_bytes[8] >= 8 * (int64_t)H,
                       "debug_op_run %s: the result buffers are too short", op);
            SearchOut out;
            SearchExtras ex;
            run_sized([&](const Ctx& cc) {
                out = SearchOut(*cc.arena, H, max_tokens);
                ex = ctc_align_device(cc, static_cast<const float*>(dev[0]), R, Tp, p, out);
            });
            K2_HIP(hipStreamSynchronize(stream_));
            K2_HIP(copy_blocking(dev[5], out.timestamps(), 4 * (size_t)H * max_tokens, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[6], ex.align_end, 4 * (size_t)H * max_tokens, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[7], ex.align_lp, 4 * (size_t)H * max_tokens, hipMemcpyDeviceToDevice));
            K2_HIP(copy_blocking(dev[8], ex.align_scores, 8 * (size_t)H, hipMemcpyDeviceToDevice));
        } else if (name == "act_forms") {
            const int act = I();
            const long long n = L();
            float *x = P(), *y_lean = P(), *y_libm = P();
            K2_REQUIRE(n >= 0 && x && y_lean && y_libm && buf_bytes[0] >= 4 * n && buf_bytes[1] >= 4 * n && buf_bytes[2] >= 4 * n,
                       "debug_op_run act_forms: three buffers of n = %lld floats are needed", n);
            act_forms(c, x, y_lean, y_libm, act, n);
        } else if (name == "ctc_prefix_beam") {
            // bufs log_probs [R][Tp][V], n_frames [R] int32 (or null), tokens [R][nbest][max_tokens] int64, timestamps (int32), token_log_probs
            //   [R][nbest][max_tokens], n_tokens [R][nbest] int32, n_hyps [R] int32, scores [R][nbest], flag [1] int32 (out); ints R, Tp, V, beam,
            //   nbest, max_tokens.  The kernel stores straight into the guarded buffers.
            K2_REQUIRE(n_bufs == 9, "debug_op_run %s: %d buffers", op, n_bufs);
            for (int k = 0; k < n_bufs; k++) P();
            const int R = I(), Tp = I(), V = I(), beam = I(), nbest = I(), max_tokens = I();
            K2_REQUIRE(!bufs[1] || buf_bytes[1] >= 4 * (int64_t)R, "debug_op_run %s: n_frames is too short", op);
            ctc_prefix_check_args(R, Tp, V, static_cast<const int32_t*>(bufs[1]), beam, nbest, max_tokens);
            const int64_t NB = (int64_t)R * nbest;
            K2_REQUIRE(dev[0] && buf_bytes[0] >= 4 * (int64_t)R * Tp * V, "debug_op_run %s: log_probs is too short", op);
            K2_REQUIRE(dev[2] && dev[3] && dev[4] && dev[5] && dev[6] && dev[7] && dev[8] && buf_bytes[2] >= 8 * NB * max_tokens &&
                           buf_bytes[3] >= 4 * NB * max_tokens && buf_bytes[4] >= 4 * NB * max_tokens && buf_bytes[5] >= 4 * NB && buf_bytes[6] >= 4 * (int64_t)R &&
                           buf_bytes[7] >= 4 * NB && buf_bytes[8] >= 4,
                       "debug_op_run %s: the result buffers are too short", op);
            CtcPrefixArgs a;
            a.log_probs = static_cast<const float*>(dev[0]); a.R = R; a.Tp = Tp; a.V = V; a.beam = beam;
            a.n_frames = static_cast<const int*>(dev[1]);
            a.nb.nbest = nbest;
            a.nb.tokens = static_cast<long long*>(dev[2]); a.nb.timestamps = static_cast<int*>(dev[3]);
            a.nb.token_log_probs = static_cast<float*>(dev[4]); a.nb.n_tokens = static_cast<int*>(dev[5]);
            a.nb.n_hyps = static_cast<int*>(dev[6]); a.nb.scores = static_cast<float*>(dev[7]);
            SearchOut out;
            run_sized([&](const Ctx& cc) {
                out = SearchOut(*cc.arena, R, max_tokens);
                a.nodes = cc.arena->take<int4>((int64_t)R * Tp * beam);
                a.scores = cc.arena->take<float>(R);
                a.tokens = out.tokens(); a.timestamps = out.timestamps(); a.n_tokens = out.counts(); a.max_tokens = max_tokens; a.overflow = out.flag();
                if (!cc.dry) K2_HIP(hipMemsetAsync(out.flag(), 0, sizeof(int), cc.stream));
                ctc_prefix_search(cc, a);
            });
            K2_HIP(hipStreamSynchronize(stream_));
            K2_HIP(copy_blocking(dev[8], out.flag(), 4, hipMemcpyDeviceToDevice));
        } else if (name == "ctc_prefix_beam_bias") {
            // the buffers of "ctc_prefix_beam" [0..8], then caller-supplied tables: next [S][V] int32, bonus [S][V], pending [S] (all three
            //   or none), LM states [S_lm][4] int32, arc_tok / arc_lp / arc_next [A], uni_lp / uni_next [V] (all or none; the arc buffers may
            //   be null when A = 0); ints R, Tp, V, beam, nbest, max_tokens, S, S_lm, A, start.  Everything the kernel indexes with is
            //   checked on the host first (ctc_prefix_bias_ref.h).
            K2_REQUIRE(n_bufs == 18, "debug_op_run %s: %d buffers", op, n_bufs);
            for (int k = 0; k < n_bufs; k++) P();
            const int R = I(), Tp = I(), V = I(), beam = I(), nbest = I(), max_tokens = I(), S = I(), S_lm = I();
            const long long A = L();
            const int start = I();
            K2_REQUIRE(!bufs[1] || buf_bytes[1] >= 4 * (int64_t)R, "debug_op_run %s: n_frames is too short", op);
            ctc_prefix_check_args(R, Tp, V, static_cast<const int32_t*>(bufs[1]), beam, nbest, max_tokens);
            const int64_t NB = (int64_t)R * nbest;
            K2_REQUIRE(dev[0] && buf_bytes[0] >= 4 * (int64_t)R * Tp * V, "debug_op_run %s: log_probs is too short", op);
            K2_REQUIRE(dev[2] && dev[3] && dev[4] && dev[5] && dev[6] && dev[7] && dev[8] && buf_bytes[2] >= 8 * NB * max_tokens &&
                           buf_bytes[3] >= 4 * NB * max_tokens && buf_bytes[4] >= 4 * NB * max_tokens && buf_bytes[5] >= 4 * NB && buf_bytes[6] >= 4 * (int64_t)R &&
                           buf_bytes[7] >= 4 * NB && buf_bytes[8] >= 4,
                       "debug_op_run %s: the result buffers are too short", op);
            CtcPrefixBiasTables tb;
            tb.V = V;
            if (bufs[9] || bufs[10] || bufs[11]) {
                K2_REQUIRE(S >= 1 && (int64_t)S * V <= kHotwordMaxEntries && bufs[9] && bufs[10] && bufs[11] && buf_bytes[9] >= 4 * (int64_t)S * V &&
                               buf_bytes[10] >= 4 * (int64_t)S * V && buf_bytes[11] >= 4 * (int64_t)S,
                           "debug_op_run %s: the hotword tables are incomplete or too short for S = %d", op, S);
                tb.S = S;
                tb.next = static_cast<const int32_t*>(bufs[9]); tb.bonus = static_cast<const float*>(bufs[10]); tb.pending = static_cast<const float*>(bufs[11]);
            }
            if (bufs[12] || bufs[16] || bufs[17]) {
                K2_REQUIRE(S_lm >= 1 && A >= 0 && A <= kNgramMaxArcs && bufs[12] && bufs[16] && bufs[17] && buf_bytes[12] >= 16 * (int64_t)S_lm &&
                               buf_bytes[16] >= 4 * (int64_t)V && buf_bytes[17] >= 4 * (int64_t)V &&
                               (A == 0 || (bufs[13] && bufs[14] && bufs[15] && buf_bytes[13] >= 4 * A && buf_bytes[14] >= 4 * A && buf_bytes[15] >= 4 * A)),
                           "debug_op_run %s: the LM tables are incomplete or too short for S = %d, A = %lld", op, S_lm, A);
                tb.S_lm = S_lm; tb.A = A; tb.start = start;
                tb.states = static_cast<const int32_t*>(bufs[12]);
                tb.arc_tok = static_cast<const int32_t*>(bufs[13]); tb.arc_lp = static_cast<const float*>(bufs[14]); tb.arc_next = static_cast<const int32_t*>(bufs[15]);
                tb.uni_lp = static_cast<const float*>(bufs[16]); tb.uni_next = static_cast<const int32_t*>(bufs[17]);
            }
            try {
                ctc_prefix_bias_check_tables(tb);
            } catch (const Error& e) {   // (the caller's tables, not a shape the launcher refuses: INVALID)
                failf(K2HIP_ERR_INVALID, "debug_op_run %s: %s", op, e.what());
            }
            CtcPrefixBiasArgs a;
            a.log_probs = static_cast<const float*>(dev[0]); a.R = R; a.Tp = Tp; a.V = V; a.beam = beam;
            a.n_frames = static_cast<const int*>(dev[1]);
            a.nb.nbest = nbest;
            a.nb.tokens = static_cast<long long*>(dev[2]); a.nb.timestamps = static_cast<int*>(dev[3]);
            a.nb.token_log_probs = static_cast<float*>(dev[4]); a.nb.n_tokens = static_cast<int*>(dev[5]);
            a.nb.n_hyps = static_cast<int*>(dev[6]); a.nb.scores = static_cast<float*>(dev[7]);
            if (tb.next) a.hw = BeamHwStream{static_cast<const int*>(dev[9]), static_cast<const float*>(dev[10]), static_cast<const float*>(dev[11])};
            if (tb.states) {
                a.lm.states = static_cast<const int4*>(dev[12]);
                a.lm.arc_tok = static_cast<const int*>(dev[13]); a.lm.arc_lp = static_cast<const float*>(dev[14]); a.lm.arc_next = static_cast<const int*>(dev[15]);
                a.lm.uni_lp = static_cast<const float*>(dev[16]); a.lm.uni_next = static_cast<const int*>(dev[17]);
                a.lm.start = start;
            }
            SearchOut out;
            run_sized([&](const Ctx& cc) {
                out = SearchOut(*cc.arena, R, max_tokens);
                a.nodes = cc.arena->take<int4>((int64_t)R * Tp * beam);
                a.scores = cc.arena->take<float>(R);
                a.tokens = out.tokens(); a.timestamps = out.timestamps(); a.n_tokens = out.counts(); a.max_tokens = max_tokens; a.overflow = out.flag();
                if (!cc.dry) K2_HIP(hipMemsetAsync(out.flag(), 0, sizeof(int), cc.stream));
                ctc_prefix_search_biased(cc, a);
            });
            K2_HIP(hipStreamSynchronize(stream_));
            K2_HIP(copy_blocking(dev[8], out.flag(), 4, hipMemcpyDeviceToDevice));
        } else if (name == "ctc_prefix_resume") {
            // bufs log_probs [B][Tc][V], n_frames [B] int32 (or null), in [B][in_ints] (caller-supplied), out [B][out_ints], status [1] int32
            //   (out); ints B, Tc, V, beam.  The kernel stores straight into the guarded buffers.
            K2_REQUIRE(n_bufs == 5, "debug_op_run %s: %d buffers", op, n_bufs);
            for (int k = 0; k < n_bufs; k++) P();
            const int B = I(), Tc = I(), V = I(), beam = I();
            K2_REQUIRE(B >= 1 && Tc >= 1 && V >= 1 && beam >= 1 && beam <= kMaxBeam, "debug_op_run %s: bad shape", op);
            const CtcPrefixResumeLayout RL{beam, Tc};
            K2_REQUIRE(!bufs[1] || buf_bytes[1] >= 4 * (int64_t)B, "debug_op_run %s: n_frames is too short", op);
            K2_REQUIRE(bufs[2] && buf_bytes[2] >= 4 * (int64_t)B * RL.in_ints(), "debug_op_run %s: the in blocks are too short", op);
            ctc_prefix_chunk_check_args(B, Tc, V, static_cast<const int32_t*>(bufs[1]), beam, static_cast<const int*>(bufs[2]), RL.in_ints(), RL.in_e(), RL.in_rel());
            K2_REQUIRE(dev[0] && buf_bytes[0] >= 4 * (int64_t)B * Tc * V, "debug_op_run %s: log_probs is too short", op);
            K2_REQUIRE(dev[3] && dev[4] && buf_bytes[3] >= 4 * (int64_t)B * RL.out_ints() && buf_bytes[4] >= 4, "debug_op_run %s: the result buffers are too short", op);
            CtcPrefixResumeArgs a;
            a.log_probs = static_cast<const float*>(dev[0]); a.B = B; a.Tc = Tc; a.V = V; a.beam = beam;
            a.n_frames = static_cast<const int*>(dev[1]);
            a.in = static_cast<const int*>(dev[2]); a.out = static_cast<int*>(dev[3]); a.status = static_cast<int*>(dev[4]);
            K2_HIP(hipMemsetAsync(dev[4], 0, sizeof(int), stream_));
            run_sized([&](const Ctx& cc) {
                a.nodes = cc.arena->take<int4>((int64_t)B * Tc * beam);
                ctc_prefix_resume(cc, a);
            });
        } else if (name == "ctc_prefix_resume_bias") {
            // the buffers of "ctc_prefix_resume" [0..4], side in [B][1 + 3K] (caller-supplied) [5], side out [B][5K] (out) [6], the nine table
            //   buffers of "ctc_prefix_beam_bias" [7..15] (one set per call), row_graph [B] int32 [16]: 1 = the row reads the hotword tables,
            //   0 = null tables for that row; ints B, Tc, V, beam, S, S_lm, A, start.  Tables and side in blocks are checked on the host first.
            K2_REQUIRE(n_bufs == 17, "debug_op_run %s: %d buffers", op, n_bufs);
            for (int k = 0; k < n_bufs; k++) P();
            const int B = I(), Tc = I(), V = I(), beam = I(), S = I(), S_lm = I();
            const long long A = L();
            const int start = I();
            K2_REQUIRE(B >= 1 && Tc >= 1 && V >= 1 && beam >= 1 && beam <= kMaxBeam, "debug_op_run %s: bad shape", op);
            const CtcPrefixResumeLayout RL{beam, Tc};
            const CtcPrefixResumeBiasLayout SL{beam};
            K2_REQUIRE(!bufs[1] || buf_bytes[1] >= 4 * (int64_t)B, "debug_op_run %s: n_frames is too short", op);
            K2_REQUIRE(bufs[2] && buf_bytes[2] >= 4 * (int64_t)B * RL.in_ints(), "debug_op_run %s: the in blocks are too short", op);
            ctc_prefix_chunk_check_args(B, Tc, V, static_cast<const int32_t*>(bufs[1]), beam, static_cast<const int*>(bufs[2]), RL.in_ints(), RL.in_e(), RL.in_rel());
            K2_REQUIRE(dev[0] && buf_bytes[0] >= 4 * (int64_t)B * Tc * V, "debug_op_run %s: log_probs is too short", op);
            K2_REQUIRE(dev[3] && dev[4] && dev[6] && buf_bytes[3] >= 4 * (int64_t)B * RL.out_ints() && buf_bytes[4] >= 4 && buf_bytes[6] >= 4 * (int64_t)B * SL.out_ints(),
                       "debug_op_run %s: the result buffers are too short", op);
            K2_REQUIRE(bufs[5] && buf_bytes[5] >= 4 * (int64_t)B * SL.in_ints() && bufs[16] && buf_bytes[16] >= 4 * (int64_t)B,
                       "debug_op_run %s: the side in blocks or row_graph are too short", op);
            CtcPrefixBiasTables tb;
            tb.V = V;
            if (bufs[7] || bufs[8] || bufs[9]) {
                K2_REQUIRE(S >= 1 && (int64_t)S * V <= kHotwordMaxEntries && bufs[7] && bufs[8] && bufs[9] && buf_bytes[7] >= 4 * (int64_t)S * V &&
                               buf_bytes[8] >= 4 * (int64_t)S * V && buf_bytes[9] >= 4 * (int64_t)S,
                           "debug_op_run %s: the hotword tables are incomplete or too short for S = %d", op, S);
                tb.S = S;
                tb.next = static_cast<const int32_t*>(bufs[7]); tb.bonus = static_cast<const float*>(bufs[8]); tb.pending = static_cast<const float*>(bufs[9]);
            }
            if (bufs[10] || bufs[14] || bufs[15]) {
                K2_REQUIRE(S_lm >= 1 && A >= 0 && A <= kNgramMaxArcs && bufs[10] && bufs[14] && bufs[15] && buf_bytes[10] >= 16 * (int64_t)S_lm &&
                               buf_bytes[14] >= 4 * (int64_t)V && buf_bytes[15] >= 4 * (int64_t)V &&
                               (A == 0 || (bufs[11] && bufs[12] && bufs[13] && buf_bytes[11] >= 4 * A && buf_bytes[12] >= 4 * A && buf_bytes[13] >= 4 * A)),
                           "debug_op_run %s: the LM tables are incomplete or too short for S = %d, A = %lld", op, S_lm, A);
                tb.S_lm = S_lm; tb.A = A; tb.start = start;
                tb.states = static_cast<const int32_t*>(bufs[10]);
                tb.arc_tok = static_cast<const int32_t*>(bufs[11]); tb.arc_lp = static_cast<const float*>(bufs[12]); tb.arc_next = static_cast<const int32_t*>(bufs[13]);
                tb.uni_lp = static_cast<const float*>(bufs[14]); tb.uni_next = static_cast<const int32_t*>(bufs[15]);
            }
            const int32_t* row_graph = static_cast<const int32_t*>(bufs[16]);
            try {
                ctc_prefix_bias_check_tables(tb);
                for (int b = 0; b < B; b++) {
                    K2_REQUIRE(row_graph[b] == 0 || (row_graph[b] == 1 && tb.next), "row_graph[%d] = %d (hotword tables: %s)", b, row_graph[b], tb.next ? "given" : "none");
                    ctc_prefix_bias_check_side_in(static_cast<const int*>(bufs[5]) + (size_t)b * (size_t)SL.in_ints(), beam, row_graph[b] ? tb.S : 0,
                                                  tb.states ? tb.S_lm : 0, b);
                }
            } catch (const Error& e) {   // (the caller's tables and blocks, not a shape the launcher refuses: INVALID)
                failf(K2HIP_ERR_INVALID, "debug_op_run %s: %s", op, e.what());
            }
            std::vector<BeamHwStream> hws((size_t)B);
            for (int b = 0; b < B; b++)
                if (row_graph[b]) hws[(size_t)b] = BeamHwStream{static_cast<const int*>(dev[7]), static_cast<const float*>(dev[8]), static_cast<const float*>(dev[9])};
            BeamHwStream* d_hws = nullptr;
            K2_HIP(hipMalloc(&d_hws, sizeof(BeamHwStream) * (size_t)B));
            d.base.push_back(reinterpret_cast<char*>(d_hws));
            K2_HIP(copy_blocking(d_hws, hws.data(), sizeof(BeamHwStream) * (size_t)B, hipMemcpyHostToDevice));
            CtcPrefixResumeBiasArgs a;
            a.log_probs = static_cast<const float*>(dev[0]); a.B = B; a.Tc = Tc; a.V = V; a.beam = beam;
            a.n_frames = static_cast<const int*>(dev[1]);
            a.in = static_cast<const int*>(dev[2]); a.out = static_cast<int*>(dev[3]); a.status = static_cast<int*>(dev[4]);
            a.side_in = static_cast<const int*>(dev[5]); a.side_out = static_cast<int*>(dev[6]);
            a.hw_streams = d_hws;
            if (tb.states) {
                a.lm.states = static_cast<const int4*>(dev[10]);
                a.lm.arc_tok = static_cast<const int*>(dev[11]); a.lm.arc_lp = static_cast<const float*>(dev[12]); a.lm.arc_next = static_cast<const int*>(dev[13]);
                a.lm.uni_lp = static_cast<const float*>(dev[14]); a.lm.uni_next = static_cast<const int*>(dev[15]);
                a.lm.start = start;
            }
            K2_HIP(hipMemsetAsync(dev[4], 0, sizeof(int), stream_));
            run_sized([&](const Ctx& cc) {
                a.nodes = cc.arena->take<int4>((int64_t)B * Tc * beam);
                ctc_prefix_resume_biased(cc, a);
            });
        } else if (name == "basicnorm") {
            float *x = P(), *le = P(), *y = P();
            const int M = I(), D = I();
            basicnorm(c, x, le, y, M, D);
        } else if (name == "conv0_pad1_dswish" || name == "conv0_nopad_dswish" || name == "conv0_swoosh") {
            float *x = P(), *w = P(), *b = P(), *y = P();
            const int B = I(), T = I(), Fq = I();
            if (name == "conv0_pad1_dswish") conv0_pad1_dswish(c, x, w, b, y, B, T, Fq);
            else if (name == "conv0_nopad_dswish") conv0_nopad_dswish(c, x, w, b, y, B, T, Fq);
            else conv0_swoosh(c, x, w, b, y, B, T, Fq);
        } else if (name == "pad_logfloor") {
            float* packed = P();
            const long long *off = reinterpret_cast<const long long*>(P()), *len = reinterpret_cast<const long long*>(P());
            float* out = P();
            const int B = I();
            const long long Lf = L();
            pad_logfloor(c, packed, off, len, out, B, Lf);
        } else if (name == "pad_logfloor_dense") {
            float* feats = P();
            const long long n_each = L();
            float* out = P();
            const int B = I();
            const long long Lf = L();
            pad_logfloor_dense(c, feats, n_each, out, B, Lf);
        } else if (name == "gather_samples") {
            // ints B, nmax, off[0 .. B): the float offset of every stream's source inside the samples buffer (the device table of
            // source pointers is built here); bufs samples, n (int64 [B]), dst
            const int B = I();
            const long long nmax = L();
            K2_REQUIRE(B > 0 && B <= 64, "debug_op_run gather_samples: B = %d", B);
            std::vector<long long> off((size_t)B);
            for (auto& o : off) o = L();
            float* samples = P();
            const long long* n = reinterpret_cast<const long long*>(P());
            float* dst = P();
            K2_REQUIRE(samples && n && dst && buf_bytes[1] >= 8 * (int64_t)B, "debug_op_run gather_samples: three buffers are needed");
            std::vector<const float*> h((size_t)B);
            for (int b = 0; b < B; b++) {
                K2_REQUIRE(off[(size_t)b] >= 0 && 4 * off[(size_t)b] <= buf_bytes[0], "debug_op_run gather_samples: offset %lld", off[(size_t)b]);
                h[(size_t)b] = samples + off[(size_t)b];
            }
            const float** table = nullptr;
            K2_HIP(hipMalloc(&table, sizeof(float*) * (size_t)B));
            d.base.push_back(reinterpret_cast<char*>(table));
            K2_HIP(copy_blocking(table, h.data(), sizeof(float*) * (size_t)B, hipMemcpyHostToDevice));
            gather_samples(c, table, n, dst, B, nmax);
        } else if (name == "resample_gather") {
            // ints B, n_dst_rows, nmax, then per row (in_rate, out_rate, off_head, n_head, off_tail, n_tail, x0, k0, n_out, dst_row) --
            // in_rate = 0: a pass-through row; the offsets are floats into the samples buffer; bufs samples, dst [n_dst_rows][nmax].
            // The plans are built and uploaded here (tables freed with the call); the launcher checks every row's extents.
            const int B = I(), n_dst = I();
            const long long nmax = L();
            K2_REQUIRE(B > 0 && B <= 64 && n_dst > 0 && nmax > 0, "debug_op_run resample_gather: B = %d, rows = %d, nmax = %lld", B, n_dst, nmax);
            std::vector<long long> ia((size_t)B * 10);
            for (auto& v : ia) v = L();
            float* samples = P();
            float* dst = P();
            K2_REQUIRE(samples && dst && buf_bytes[1] >= 4 * (int64_t)n_dst * nmax, "debug_op_run resample_gather: two buffers are needed, dst of %d x %lld floats",
                       n_dst, nmax);
            std::vector<ResampleRow> rows((size_t)B);
            for (int b = 0; b < B; b++) {
                const long long* a = ia.data() + (size_t)b * 10;
                K2_REQUIRE(a[2] >= 0 && a[3] >= 0 && a[4] >= 0 && a[5] >= 0 && 4 * (a[2] + a[3]) <= buf_bytes[0] && 4 * (a[4] + a[5]) <= buf_bytes[0],
                           "debug_op_run resample_gather: row %d: pieces %lld + %lld and %lld + %lld floats", b, a[2], a[3], a[4], a[5]);
                ResampleRow& r = rows[(size_t)b];
                r.head = samples + a[2]; r.n_head = a[3]; r.tail = samples + a[4]; r.n_tail = a[5];
                r.dst_row = (int)a[9];
                if (a[0] == 0) continue;
                const ResamplePlan p = resample_plan((int)a[0], (int)a[1]);
                const size_t nw = p.w.size(), no = (size_t)p.ou;
                char* t = nullptr;
                K2_HIP(hipMalloc(&t, 4 * (nw + 2 * no)));
                d.base.push_back(t);
                K2_HIP(copy_blocking(t, p.w.data(), 4 * nw, hipMemcpyHostToDevice));
                K2_HIP(copy_blocking(t + 4 * nw, p.first.data(), 4 * no, hipMemcpyHostToDevice));
                K2_HIP(copy_blocking(t + 4 * (nw + no), p.ntaps.data(), 4 * no, hipMemcpyHostToDevice));
                r.w = reinterpret_cast<const float*>(t); r.first = reinterpret_cast<const int*>(t + 4 * nw); r.ntaps = r.first + no;
                r.iu = p.iu; r.ou = p.ou; r.max_taps = p.max_taps; r.wmax = p.wmax;
                r.x0 = a[6]; r.k0 = a[7]; r.n_out = a[8];
            }
            ResampleRow* d_rows = nullptr;
            K2_HIP(hipMalloc(&d_rows, sizeof(ResampleRow) * (size_t)B));
            d.base.push_back(reinterpret_cast<char*>(d_rows));
            K2_HIP(copy_blocking(d_rows, rows.data(), sizeof(ResampleRow) * (size_t)B, hipMemcpyHostToDevice));
            resample_gather(c, rows.data(), d_rows, B, dst, n_dst, nmax);
        } else if (name == "rnn_lm_embed") {
            const long long R = L();
            const int E = I();
            float* emb = P();
            const int* ids = reinterpret_cast<const int*>(P());
            float* x0 = P();
            K2_REQUIRE(emb && ids && x0 && R > 0 && buf_bytes[1] >= 4 * R && buf_bytes[2] >= 4 * R * E, "debug_op_run rnn_lm_embed: %lld rows need ids and x0", R);
            for (long long i = 0; i < R; i++)   // (the launcher trusts its ids: checked here on the caller's copy)
                K2_REQUIRE(E > 0 && static_cast<const int*>(bufs[1])[i] >= 0 && 4LL * E * (static_cast<const int*>(bufs[1])[i] + 1LL) <= buf_bytes[0],
                           "debug_op_run rnn_lm_embed: id %d of row %lld is outside the embedding", static_cast<const int*>(bufs[1])[i], i);
            rnn_lm_embed(c, emb, ids, x0, R, E);
        } else if (name == "rnn_lm_step") {
            const int a = I(), H = I(), first = I();
            float *hp = P(), *w = P(), *gx = P(), *cc = P(), *ho = P();
            K2_REQUIRE(hp && w && gx && cc && ho && a > 0 && H > 0 && buf_bytes[0] >= 4LL * a * H && buf_bytes[1] >= 16LL * H * H && buf_bytes[2] >= 16LL * a * H &&
                           buf_bytes[3] >= 4LL * a * H && buf_bytes[4] >= 4LL * a * H,
                       "debug_op_run rnn_lm_step: the buffers are short of %d rows of hidden_dim %d", a, H);
            rnn_lm_step(c, first ? nullptr : hp, w, gx, cc, ho, a, H);
        } else if (name == "rnn_lm_score") {
            const long long R = L();
            const int H = I(), V = I(), Vp = I();
            float *y = P(), *okn = P(), *ob = P();
            const int* tgt = reinterpret_cast<const int*>(P());
            float* lp = P();
            K2_REQUIRE(y && okn && ob && tgt && lp && R > 0 && H > 0 && V > 0 && Vp >= V && buf_bytes[0] >= 4 * R * H && buf_bytes[1] >= 4LL * H * Vp &&
                           buf_bytes[2] >= 4LL * V && buf_bytes[3] >= 4 * R && buf_bytes[4] >= 4 * R,
                       "debug_op_run rnn_lm_score: the buffers are short of %lld rows, hidden_dim %d, %d columns", R, H, Vp);
            for (long long i = 0; i < R; i++)
                K2_REQUIRE(static_cast<const int*>(bufs[3])[i] >= 0 && static_cast<const int*>(bufs[3])[i] < V, "debug_op_run rnn_lm_score: target %d of row %lld",
                           static_cast<const int*>(bufs[3])[i], i);
            rnn_lm_score_rows(c, y, okn, ob, tgt, lp, R, H, V, Vp);
        } else if (name == "nlm_advance") {
            // ints M, in, H, use_emb, V (rows of emb), live (-1: no flag, else the flag's value)
            const int M = I(), in = I(), H = I(), use_emb = I(), V = I(), live = I();
            float *wcat = P(), *bias = P(), *x = P(), *hp = P(), *cp = P(), *ho = P(), *co = P();
            const int* par = reinterpret_cast<const int*>(P());
            const int* tok = reinterpret_cast<const int*>(P());
            int* flag = reinterpret_cast<int*>(P());
            long long* work = reinterpret_cast<long long*>(P());
            K2_REQUIRE(M > 0 && in > 0 && H > 0 && V > 0, "debug_op_run nlm_advance: bad shape");
            const long long Kc = (in + 31) / 32 * 32 + H, xrows = use_emb ? V : M;
            K2_REQUIRE(wcat && bias && x && hp && cp && ho && co && par && tok && flag && work && buf_bytes[0] >= 16LL * H * Kc && buf_bytes[1] >= 16LL * H &&
                           buf_bytes[2] >= 4LL * xrows * in && buf_bytes[3] >= 4LL * M * H && buf_bytes[4] >= 4LL * M * H && buf_bytes[5] >= 4LL * M * H &&
                           buf_bytes[6] >= 4LL * M * H && buf_bytes[7] >= 4LL * M && buf_bytes[8] >= 4LL * M && buf_bytes[9] >= 4 && buf_bytes[10] >= 16,
                       "debug_op_run nlm_advance: the buffers are short of %d rows, input %d, hidden_dim %d", M, in, H);
            for (int i = 0; i < M; i++) {   // (the launcher trusts its indexes: checked here on the caller's copy)
                const int p = static_cast<const int*>(bufs[7])[i], t = static_cast<const int*>(bufs[8])[i];
                K2_REQUIRE(p >= 0 && p < M && t >= -1 && (use_emb ? t < V : true), "debug_op_run nlm_advance: row %d continues slot %d with token %d", i, p, t);
            }
            if (live >= 0) K2_HIP(hipMemsetD32Async((hipDeviceptr_t)flag, live, 1, stream_));
            NlmAdvance a;
            a.wcat = wcat; a.bias = bias;
            a.emb = use_emb ? x : nullptr; a.x_rows = use_emb ? nullptr : x;
            a.h_par = hp; a.c_par = cp; a.h_out = ho; a.c_out = co;
            a.par = par; a.tok = tok; a.live = live >= 0 ? flag : nullptr; a.work = work;
            a.M = M; a.in = in; a.H = H;
            nlm_advance(c, a);
        } else if (name == "nlm_rows") {
            // ints M, H, V, live (-1: no flag)
            const int M = I(), H = I(), V = I(), live = I();
            float *h = P(), *wout = P(), *ob = P(), *qp = P(), *qo = P();
            const int* par = reinterpret_cast<const int*>(P());
            const int* tok = reinterpret_cast<const int*>(P());
            int* flag = reinterpret_cast<int*>(P());
            K2_REQUIRE(M > 0 && H > 0 && V > 0 && h && wout && ob && qp && qo && par && tok && flag && buf_bytes[0] >= 4LL * M * H && buf_bytes[1] >= 4LL * V * H &&
                           buf_bytes[2] >= 4LL * V && buf_bytes[3] >= 4LL * M * V && buf_bytes[4] >= 4LL * M * V && buf_bytes[5] >= 4LL * M &&
                           buf_bytes[6] >= 4LL * M && buf_bytes[7] >= 4,
                       "debug_op_run nlm_rows: the buffers are short of %d rows, hidden_dim %d, V = %d", M, H, V);
            for (int i = 0; i < M; i++)
                K2_REQUIRE(static_cast<const int*>(bufs[5])[i] >= 0 && static_cast<const int*>(bufs[5])[i] < M, "debug_op_run nlm_rows: row %d continues slot %d", i,
                           static_cast<const int*>(bufs[5])[i]);
            if (live >= 0) K2_HIP(hipMemsetD32Async((hipDeviceptr_t)flag, live, 1, stream_));
            nlm_rows(c, h, wout, ob, qp, qo, par, tok, live >= 0 ? flag : nullptr, M, H, V);
        } else if (name == "nlm_load_streams" || name == "nlm_store_streams") {
            // ints B, K, L, H, V; bufs blocks [B][NlmStreamLayout::block_floats()], cur [B] (int32: the current half, -1: no state yet),
            // then (load) nh [B] (int32), h0 [L][H], c0 [L][H], q0 [V], h [L][M][H] (out), c (out), q [M][V] (out), io [B] x 16 bytes (scratch)
            //      (store) h, c, q, io: the call writes the OTHER half of every block (half 0 of a block without a state)
            const bool load = name == "nlm_load_streams";
            const int B = I(), K = I(), Ln = I(), H = I(), V = I();
            K2_REQUIRE(B > 0 && B <= 4096 && K >= 1 && K <= kMaxBeam && Ln >= 1 && Ln <= 8 && H > 0 && H % 4 == 0 && V > 0, "debug_op_run %s: bad shape", op);
            const NlmStreamLayout lay{K, Ln, H, V};
            const long long M = (long long)B * K;
            float* blocks = P();
            const int* cur = reinterpret_cast<const int*>(P());
            const int* nh = load ? reinterpret_cast<const int*>(P()) : nullptr;
            float *h0 = load ? P() : nullptr, *c0 = load ? P() : nullptr, *q0 = load ? P() : nullptr;
            float *h = P(), *cc = P(), *q = P();
            NlmStreamIO* io = reinterpret_cast<NlmStreamIO*>(P());
            const int o = load ? 6 : 2;   // index of h among the buffers
            K2_REQUIRE(blocks && cur && h && cc && q && io && (!load || (nh && h0 && c0 && q0)) && buf_bytes[0] >= 4LL * B * lay.block_floats() && buf_bytes[1] >= 4LL * B &&
                           buf_bytes[o] >= 4LL * Ln * M * H && buf_bytes[o + 1] >= 4LL * Ln * M * H && buf_bytes[o + 2] >= 4LL * M * V &&
                           buf_bytes[o + 3] >= (long long)sizeof(NlmStreamIO) * B &&
                           (!load || (buf_bytes[2] >= 4LL * B && buf_bytes[3] >= 4LL * Ln * H && buf_bytes[4] >= 4LL * Ln * H && buf_bytes[5] >= 4LL * V)),
                       "debug_op_run %s: the buffers are short of %d streams, beam %d, %d layers of %d, V = %d", op, B, K, Ln, H, V);
            std::vector<NlmStreamIO> tbl((size_t)B);
            for (int b = 0; b < B; b++) {
                const int cb = static_cast<const int*>(bufs[1])[b];
                K2_REQUIRE(cb >= -1 && cb <= 1, "debug_op_run %s: stream %d names half %d", op, b, cb);
                K2_REQUIRE(!load || (static_cast<const int*>(bufs[2])[b] >= 0 && static_cast<const int*>(bufs[2])[b] <= K), "debug_op_run %s: stream %d has %d hypotheses", op,
                           b, load ? static_cast<const int*>(bufs[2])[b] : 0);
                float* base = blocks + (long long)b * lay.block_floats();
                tbl[(size_t)b].rd = cb < 0 ? nullptr : base + cb * lay.half_floats();
                tbl[(size_t)b].wr = base + (cb < 0 ? 0 : (cb ^ 1)) * lay.half_floats();
            }
            K2_HIP(copy_blocking(io, tbl.data(), sizeof(NlmStreamIO) * (size_t)B, hipMemcpyHostToDevice));
            RnnLmDev dv;
            dv.L = Ln; dv.H = H; dv.V = V;
            dv.h0 = h0; dv.c0 = c0; dv.q0 = q0;
            if (load) nlm_load_streams(c, dv, io, nh, 1, h, cc, q, B, K);
            else nlm_store_streams(c, dv, io, h, cc, q, B, K);
        } else if (name == "convnext_cat") {
            float *a3 = P(), *pool = P();
            const long long ss = L(), off = L();
            const int* slots = reinterpret_cast<const int*>(P());
            float *cat = P(), *byp = P();
            const int B = I(), T3 = I(), Tc = I(), Fq = I(), Cc = I();
            convnext_cat(c, a3, pool, ss, off, slots, cat, byp, B, T3, Tc, Fq, Cc);
        } else if (name == "cat_shift" || name == "cat_keep") {
            float* pool = P();
            const long long ss = L(), off = L();
            const int* slots = reinterpret_cast<const int*>(P());
            float* newrows = P();
            const int ldn = I();
            float* cat = P();
            const int B = I(), Lc = I(), Tc = I(), width = I(), last = I();   // last: tanh_gated (a bool as an int) / keep_back
            if (name == "cat_shift") cat_shift(c, pool, ss, off, slots, newrows, ldn, cat, B, Lc, Tc, width, last != 0);
            else cat_keep(c, pool, ss, off, slots, newrows, ldn, cat, B, Lc, Tc, width, last);
        } else if (name == "fifo_append") {
            float* fifo = P();
            const int cap = I(), feat = I();
            float* src = P();
            const int *slots = reinterpret_cast<const int*>(P()), *pos = reinterpret_cast<const int*>(P());
            const int G = I(), nf = I();
            fifo_append(c, fifo, cap, feat, src, slots, pos, G, nf);
        } else if (name == "fifo_gather") {
            float* fifo = P();
            const int cap = I(), feat = I();
            const int *slots = reinterpret_cast<const int*>(P()), *head = reinterpret_cast<const int*>(P());
            float* x = P();
            const int B = I(), T = I();
            fifo_gather(c, fifo, cap, feat, slots, head, x, B, T);
        } else if (name == "zero_floats" || name == "logfloor_inplace") {
            float* p = P();
            const long long n = L();
            if (name == "zero_floats") zero_floats(c, p, n);
            else logfloor_inplace(c, p, n);
        } else if (name == "glu_sigmoid" || name == "tanh_gate") {
            float *x = P(), *y = P();
            const int M = I(), D = I();
            if (name == "glu_sigmoid") glu_sigmoid(c, x, y, M, D);
            else tanh_gate(c, x, y, M, D);
        } else if (name == "convert_channels") {
            float *x = P(), *y = P();
            const int M = I(), Din = I(), Dout = I();
            convert_channels(c, x, y, M, Din, Dout);
        } else if (name == "copy_cols") {
            float* x = P();
            const int ldx = I(), xcol0 = I();
            float* y = P();
            const int ldy = I(), ycol0 = I(), M = I(), n = I();
            copy_cols(c, x, ldx, xcol0, y, ldy, ycol0, M, n);
        } else if (name == "tanh_add") {
            float *enc = P(), *dec = P();
            const int dec_stride = I();
            float* y = P();
            const int N = I(), J = I();
            tanh_add(c, enc, dec, dec_stride, y, N, J);
        } else if (name == "argmax_rows" || name == "argmax_first_rows") {
            float* logits = P();
            const int ld = I(), N = I(), V = I();
            int* tok = reinterpret_cast<int*>(P());
            if (name == "argmax_rows") argmax_rows(c, logits, ld, N, V, tok);
            else argmax_first_rows(c, logits, ld, N, V, tok);
        } else if (name == "log_softmax_rows") {
            float* x = P();
            const int M = I(), V = I();
            log_softmax_rows(c, x, M, V);
        } else if (name == "ctc_collapse") {
            const int* tok = reinterpret_cast<const int*>(P());
            const int B = I(), Tp = I();
            const int* frame_off = reinterpret_cast<const int*>(P());
            long long* tokens = reinterpret_cast<long long*>(P());
            int *timestamps = reinterpret_cast<int*>(P()), *n_tokens = reinterpret_cast<int*>(P());
            const int max_tokens = I();
            int *trail = reinterpret_cast<int*>(P()), *any = reinterpret_cast<int*>(P()), *overflow = reinterpret_cast<int*>(P());
            ctc_collapse(c, tok, B, Tp, frame_off, tokens, timestamps, n_tokens, max_tokens, trail, any, overflow);
        } else if (name == "first_emit_frame") {
            const int* tok = reinterpret_cast<const int*>(P());
            const int B = I(), Tp = I(), skip1 = I();
            int* t0 = reinterpret_cast<int*>(P());
            first_emit_frame(c, tok, B, Tp, skip1, t0);
        } else {
            failf(K2HIP_ERR_INVALID, "debug_op_run: unknown op '%s'", op);
        }
    } catch (const Error& e) {
        // a shape the launcher refuses; argument-count mistakes of the caller stay INVALID
        if (e.code == K2HIP_ERR_INVALID && strncmp(e.what(), "debug_op_run", 12) != 0) throw Error(K2HIP_ERR_UNSUPPORTED, e.what());
        throw;
    }
    if (!took) failf(K2HIP_ERR_UNSUPPORTED, "debug_op_run %s: the launcher does not take this shape", op);
    K2_REQUIRE(ni == n_iargs && nbuf == n_bufs, "debug_op_run %s: %d int arguments and %d buffers passed, %d and %d used", op, n_iargs, n_bufs, ni,
               nbuf);
    K2_HIP(hipStreamSynchronize(stream_));
    std::vector<unsigned char> g((size_t)kGuard);
    for (int k = 0; k < n_bufs; k++) {
        if (!dev[k]) continue;
        const char* p = static_cast<const char*>(dev[k]);
        for (int side = 0; side < 2; side++) {
            K2_HIP(copy_blocking(g.data(), side ? p + buf_bytes[k] : p - kGuard, (size_t)kGuard, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < kGuard; i++)
                if (g[(size_t)i] != 0xff)
                    failf(K2HIP_ERR_INVALID, "debug_op_run %s: buffer %d written %s its end (guard byte %lld)", op, k, side ? "past" : "before",
                          (long long)(side ? i : kGuard - i));
        }
    }
    for (int k = 0; k < n_bufs; k++)
        if (dev[k] && (out_mask >> k & 1u)) K2_HIP(copy_blocking(bufs[k], dev[k], (size_t)buf_bytes[k], hipMemcpyDeviceToHost));
}

// tuning hook: ONE launch of the LDS-DMA, ring or pipelined kernel that cfg forces, with in-kernel s_memtime stamps; out [n_wg][n_waves][64]
void Engine::debug_gemm_trace(int M, int N, int K, int act, bool with_res, int cfg, unsigned long long* out, int64_t cap, int* n_wg, int* n_waves) {
    K2_HIP(hipSetDevice(device_));
    GemmForceGuard force(cfg);
    GemmArgs g;
    g.lda = K; g.ldw = K; g.ldc = N; g.M = M; g.N = N; g.K = K; g.act = act; g.ldr = N;
    const GemmPlan p = plan_gemm(g, gemm_force());
    K2_REQUIRE(p.family == GemmFamily::DMA || p.family == GemmFamily::RING || p.family == GemmFamily::PIPE,
               "trace: LDS-DMA (0, 5, 7, 9, 10, 11), ring (100+) and pipelined (2000+) configurations only");
    *n_wg = cdiv(M, p.BM) * cdiv(N, p.BN);
    *n_waves = p.waves;
    const int64_t words = (int64_t)*n_wg * p.waves * 64;
    K2_REQUIRE(words <= cap, "trace buffer too small: need %lld words", (long long)words);
    std::vector<float> h((size_t)std::max((int64_t)M * K, std::max((int64_t)N * K, (int64_t)M * N)));
    uint32_t s = 12345u;
    for (auto& v : h) { s = s * 1664525u + 1013904223u; v = ((s >> 8) * (1.0f / 8388608.0f)) - 1.0f; }
    DevBufs dev;
    float* A = dev.alloc<float>((size_t)M * K);
    float* W = dev.alloc<float>((size_t)N * K);
    float* C = dev.alloc<float>((size_t)M * N);
    float* b = dev.alloc<float>((size_t)N);
    unsigned long long* dbg = dev.alloc<unsigned long long>((size_t)cap);
    K2_HIP(fill_blocking(dbg, 0, sizeof(unsigned long long) * (size_t)cap));
    K2_HIP(copy_blocking(A, h.data(), sizeof(float) * (size_t)M * K, hipMemcpyHostToDevice));
    K2_HIP(copy_blocking(W, h.data(), sizeof(float) * (size_t)N * K, hipMemcpyHostToDevice));
    K2_HIP(copy_blocking(C, h.data(), sizeof(float) * (size_t)M * N, hipMemcpyHostToDevice));
    K2_HIP(copy_blocking(b, h.data(), sizeof(float) * (size_t)N, hipMemcpyHostToDevice));
    Ctx c = make_ctx(false);
    c.instrument = false;
    c.stats = nullptr;
    g.A = A; g.W = W; g.bias = b; g.C = C; g.res = with_res ? C : nullptr;
    for (int i = 0; i < 5; i++) gemm(c, g);   // steady state (caches, clocks)
    g.dbg = dbg;
    gemm(c, g);
    K2_HIP(hipStreamSynchronize(stream_));
    K2_HIP(copy_blocking(out, dbg, sizeof(unsigned long long) * (size_t)words, hipMemcpyDeviceToHost));
}

void* Engine::dev_alloc(int64_t bytes) {
    K2_HIP(hipSetDevice(device_));
    void* p = nullptr;
    K2_HIP(hipMalloc(&p, (size_t)bytes));
    return p;
}
void Engine::dev_free(void* p) {
    K2_HIP(hipSetDevice(device_));
    K2_HIP(hipFree(p));
}
void Engine::dev_upload(void* dst, const void* src, int64_t bytes) {
    K2_HIP(hipSetDevice(device_));
    K2_HIP(copy_blocking(dst, src, (size_t)bytes, hipMemcpyHostToDevice));
}
void* Engine::host_alloc(int64_t bytes) {
    K2_HIP(hipSetDevice(device_));
    void* p = nullptr;
    K2_HIP(hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault));
    return p;
}
void Engine::host_free(void* p) {
    K2_HIP(hipSetDevice(device_));
    K2_HIP(hipHostFree(p));
}
void Engine::synchronize() {
    K2_HIP(hipSetDevice(device_));
    K2_HIP(hipStreamSynchronize(stream_));
    if (stream2_) K2_HIP(hipStreamSynchronize(stream2_));
    for (auto& sl : slots_)
        if (sl.stream) K2_HIP(hipStreamSynchronize(sl.stream));
    // every stream this engine enqueues on -- not hipDeviceSynchronize: the work of other handles is not this call's business, and a
    // device-wide wait from one host thread while another handle records a graph is one more legacy-style operation to trip over
}

}  // namespace k2hip
