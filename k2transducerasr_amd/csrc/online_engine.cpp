// Streaming (OnlineRecognizer) path of the engine: device-resident per-stream state pool and one
// batched chunk step.  Replaces, per tick of OnlineRecognizer.ForwardBatchGreedySearch
// (OnlineRecognizer.cs:85-219): stack_states (:131) + EncoderProj (:132) + the T'-frame greedy loop
// (:141-202) + unstack_states (:204).  States never leave the GPU.
#include <climits>
#include <cmath>

#include "engine.h"
#include "ctc_prefix_ref.h"

namespace k2hip {

void Engine::online_ensure_pool() {
    if (online_pool_) return;
    const Config& c = model_->cfg();
    K2_REQUIRE(c.streaming || c.lstm, "this model is not a streaming export (metadata 'streaming' != 1)");
    OnlineLayout& L = lay_;
    long long off = 0;
    if (c.conformer) {  // OnlineProjOfConformer.GetEncoderInitStates (:55-82): cached_attn [L][left][D] then cached_conv [L][K-1][D]
        L.nl = c.nlayer[0];
        L.floats_per_stream = ((long long)c.nlayer[0] * (c.left[0] + c.kern[0] - 1) * c.dim[0] + 63) / 64 * 64;
        online_cap_ = 256;
        if (tunables().max_streams > 0) online_cap_ = tunables().max_streams;
        K2_HIP(hipSetDevice(device_));
        K2_HIP(hipMalloc(&online_pool_, sizeof(float) * (size_t)L.floats_per_stream * online_cap_));
        for (int i = online_cap_ - 1; i >= 0; i--) free_slots_.push_back(i);
        return;
    }
    if (c.lstm) {  // OnlineProjOfLstm.GetEncoderInitStates (:55-75): h [layers][d_model] then c [layers][rnn_hidden]
        L.nl = c.nlayer[0];
        L.floats_per_stream = ((long long)c.nlayer[0] * (c.dim[0] + c.rnn_hidden) + 63) / 64 * 64;
        online_cap_ = 256;
        if (tunables().max_streams > 0) online_cap_ = tunables().max_streams;
        K2_HIP(hipSetDevice(device_));
        K2_HIP(hipMalloc(&online_pool_, sizeof(float) * (size_t)L.floats_per_stream * online_cap_));
        for (int i = online_cap_ - 1; i >= 0; i--) free_slots_.push_back(i);
        return;
    }
    auto put = [&](std::vector<long long>& v, long long n) {
        v.push_back(off);
        off += (n + 3) / 4 * 4;  // keep every cache 16-byte aligned
    };
    if (c.zip1) {  // OnlineProjOfZipformer.GetEncoderInitStates (:56-111), batch 1, layer by layer
        for (int si = 0; si < c.ns; si++)
            for (int li = 0; li < c.nlayer[si]; li++) {
                const long long D = c.dim[si], A = c.att[si], left = c.left[si], K = c.kern[si];
                put(L.clen, 1);
                put(L.nonlin, D);  // cached_avg
                put(L.key, left * A);
                put(L.val1, left * (A / 2));
                put(L.val2, left * (A / 2));
                put(L.conv1, D * (K - 1));
                put(L.conv2, D * (K - 1));
                L.sizes.push_back({left * A, D, left * (A / 2), left * (A / 2), D * (K - 1), D * (K - 1)});
                L.nl++;
            }
        L.floats_per_stream = (off + 63) / 64 * 64;
        online_cap_ = 256;
        if (tunables().max_streams > 0) online_cap_ = tunables().max_streams;
        K2_HIP(hipSetDevice(device_));
        K2_HIP(hipMalloc(&online_pool_, sizeof(float) * (size_t)L.floats_per_stream * online_cap_));
        for (int i = online_cap_ - 1; i >= 0; i--) free_slots_.push_back(i);
        return;
    }
    // The four attention caches of a layer are RINGS of KL = left + Tc rows (kernels.h: RingRef): a chunk's rows overwrite the oldest
    // ones in place instead of the whole cache being rolled every chunk.  What GetEncoderInitStates / unstack_states define -- the
    // newest `left` rows in order -- is what online_read_state returns.
    const int tc50 = online_tc50();
    for (int si = 0; si < c.ns; si++) {
        const int D = c.dim[si], H = c.heads[si], left = c.left[si], kl = left + (tc50 + c.ds[si] - 1) / c.ds[si];
        for (int li = 0; li < c.nlayer[si]; li++) {
            put(L.key, (long long)kl * c.qhd[si] * H);
            put(L.nonlin, (long long)kl * (3 * D / 4));
            put(L.val1, (long long)kl * c.vhd[si] * H);
            put(L.val2, (long long)kl * c.vhd[si] * H);
            put(L.conv1, (long long)D * (c.kern[si] / 2));
            put(L.conv2, (long long)D * (c.kern[si] / 2));
            L.sizes.push_back({(long long)left * c.qhd[si] * H, (long long)left * (3 * D / 4), (long long)left * c.vhd[si] * H,
                               (long long)left * c.vhd[si] * H, (long long)D * (c.kern[si] / 2), (long long)D * (c.kern[si] / 2)});
            L.nl++;
        }
    }
    L.embed = off;
    off += 128 * 3 * 19;
    L.floats_per_stream = (off + 63) / 64 * 64;
    online_cap_ = 256;
    if (tunables().max_streams > 0) online_cap_ = tunables().max_streams;
    K2_HIP(hipSetDevice(device_));
    K2_HIP(hipMalloc(&online_pool_, sizeof(float) * (size_t)L.floats_per_stream * online_cap_));
    for (int i = online_cap_ - 1; i >= 0; i--) free_slots_.push_back(i);
}

int Engine::online_alloc_slot() {
    online_ensure_pool();
    if (!online_fifo_ && model_->cfg().feat % 4 == 0) {  // device mirror of the feature FIFOs (42 MB for 256 slots x 512 frames x 80)
        K2_HIP(hipSetDevice(device_));
        K2_HIP(hipMalloc(&online_fifo_, sizeof(float) * (size_t)online_cap_ * kFifoFrames * model_->cfg().feat));
    }
    if (free_slots_.empty())
        failf(K2HIP_ERR_CAPACITY, "all %d stream slots are in use (raise K2HIP_MAX_STREAMS before creating the model)", online_cap_);
    int slot = free_slots_.back();
    free_slots_.pop_back();
    // GetEncoderInitStates (OnlineProjOfZipformer2.cs:63-111): every cache starts at zero
    K2_HIP(hipSetDevice(device_));
    K2_HIP(hipMemsetAsync(online_pool_ + (size_t)slot * lay_.floats_per_stream, 0, sizeof(float) * (size_t)lay_.floats_per_stream, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
    return slot;
}
// host frames into ring rows pos, pos + 1, ... (mod kFifoFrames) of a slot's device FIFO (OnlineStream fed with ready-made features)
void Engine::online_fifo_write(int slot, int pos, const float* feats, int64_t n_frames) {
    if (!online_fifo_ || n_frames <= 0) return;
    K2_REQUIRE(slot >= 0 && slot < online_cap_ && pos >= 0 && pos < kFifoFrames && n_frames <= kFifoFrames, "fifo write out of range");
    const int feat = model_->cfg().feat;
    K2_HIP(hipSetDevice(device_));
    const int64_t first = std::min<int64_t>(n_frames, kFifoFrames - pos);
    float* base = online_fifo_ + (size_t)slot * kFifoFrames * feat;
    K2_HIP(copy_blocking(base + (size_t)pos * feat, feats, sizeof(float) * (size_t)first * feat, hipMemcpyHostToDevice));
    if (n_frames > first) K2_HIP(copy_blocking(base, feats + (size_t)first * feat, sizeof(float) * (size_t)(n_frames - first) * feat, hipMemcpyHostToDevice));
}
void Engine::online_free_slot(int slot) {
    if (slot >= 0) free_slots_.push_back(slot);
}

// frames of one chunk after Conv2dSubsampling + ConvNeXt (50 Hz): T = 45 -> 16
int Engine::online_tc50() const {
    const int T = model_->cfg().chunk_T, T1 = T - 2, T2 = (T1 - 3) / 2 + 1, T3 = T2 - 2;
    return T3 - 3;
}

void Engine::online_read_state(int slot, int layer, int kind, long long chunks_done, float* out, int64_t cap, int64_t* n) {
    online_ensure_pool();
    K2_REQUIRE(slot >= 0 && slot < online_cap_, "bad slot %d", slot);
    long long off, cnt;
    if (model_->cfg().conformer) {  // kind 0: cached_attn of `layer` [left, D]; kind 1: cached_conv of `layer` [K-1, D]
        const Config& cf = model_->cfg();
        K2_REQUIRE(layer >= 0 && layer < cf.nlayer[0] && (kind == 0 || kind == 1), "bad conformer state index layer=%d kind=%d", layer, kind);
        const long long na = (long long)cf.left[0] * cf.dim[0], ncv = (long long)(cf.kern[0] - 1) * cf.dim[0];
        cnt = kind == 0 ? na : ncv;
        off = kind == 0 ? layer * na : cf.nlayer[0] * na + layer * ncv;
    } else if (model_->cfg().lstm) {  // kind 0: h of `layer` [d_model]; kind 1: c of `layer` [rnn_hidden]
        const Config& cf = model_->cfg();
        K2_REQUIRE(layer >= 0 && layer < cf.nlayer[0] && (kind == 0 || kind == 1), "bad lstm state index layer=%d kind=%d", layer, kind);
        cnt = kind == 0 ? cf.dim[0] : cf.rnn_hidden;
        off = kind == 0 ? (long long)layer * cf.dim[0] : (long long)cf.nlayer[0] * cf.dim[0] + (long long)layer * cf.rnn_hidden;
    } else if (model_->cfg().zip1 && kind == 7) {  // cached_len of `layer`
        K2_REQUIRE(layer >= 0 && layer < lay_.nl, "bad state index layer=%d", layer);
        off = lay_.clen[layer];
        cnt = 1;
    } else if (kind == 6) {
        K2_REQUIRE(!model_->cfg().zip1, "a zipformer (v1) stream has no embed state");
        off = lay_.embed;
        cnt = 128 * 3 * 19;
    } else {
        K2_REQUIRE(layer >= 0 && layer < lay_.nl && kind >= 0 && kind < 6, "bad state index layer=%d kind=%d", layer, kind);
        const std::vector<long long>* v[6] = {&lay_.key, &lay_.nonlin, &lay_.val1, &lay_.val2, &lay_.conv1, &lay_.conv2};
        off = (*v[kind])[layer];
        cnt = lay_.sizes[layer][kind];
    }
    *n = cnt;
    if (!out) return;
    if (cnt > cap) failf(K2HIP_ERR_CAPACITY, "state needs %lld floats", cnt);
    K2_HIP(hipSetDevice(device_));
    K2_HIP(hipStreamSynchronize(stream_));
    const Config& cfz = model_->cfg();
    if (!cfz.conformer && !cfz.lstm && !cfz.zip1 && kind >= 0 && kind < 4) {
        // attention caches are rings: the cache the reference would hold after `chunks_done` chunks is rows Tc .. KL-1 of the last
        // [cache ; chunk] concatenation, i.e. ring rows (head + 2 Tc + j) % KL, j = 0 .. left-1, head = ((chunks_done - 1) Tc) % KL
        int si = 0, acc = 0;
        while (si < cfz.ns && layer >= acc + cfz.nlayer[si]) acc += cfz.nlayer[si++];
        const int left = cfz.left[si], tc = (online_tc50() + cfz.ds[si] - 1) / cfz.ds[si], kl = left + tc;
        const long long width = cnt / left;
        std::vector<float> ring((size_t)kl * width);
        K2_HIP(copy_blocking(ring.data(), online_pool_ + (size_t)slot * lay_.floats_per_stream + off, sizeof(float) * ring.size(), hipMemcpyDeviceToHost));
        // before the first chunk the ring is all zeros and any rotation of it is the reference's zero cache
        const long long head = chunks_done > 0 ? ((chunks_done - 1) * tc) % kl : 0;
        for (int j = 0; j < left; j++) {
            const long long p = (head + 2LL * tc + j) % kl;
            memcpy(out + (size_t)j * width, ring.data() + (size_t)p * width, sizeof(float) * (size_t)width);
        }
        return;
    }
    K2_HIP(copy_blocking(out, online_pool_ + (size_t)slot * lay_.floats_per_stream + off, sizeof(float) * (size_t)cnt, hipMemcpyDeviceToHost));
}

int Engine::online_frames_per_chunk() const {
    const Config& c = model_->cfg();
    if (c.lstm) return lstm_out_frames(c.chunk_T);
    if (c.conformer) return conformer_out_frames(c.chunk_T) - 2 - c.right;
    if (c.zip1) return ((c.chunk_T - 7) / 2 + 1) / 2;
    return (c.shift / 2 + 1) / 2;
}

// CompactRelPositionalEncoding.forward(x, left_context_len): row n <-> relative position n - (Tc+L-1)
const float* Engine::pos_emb_stream(int Tc, int L) {
    std::lock_guard<std::mutex> lk(cache_mu_);
    const int key = -(Tc * 100000 + L);  // negative keys: streaming tables
    auto it = pe_cache_.find(key);
    if (it != pe_cache_.end()) return it->second;
    const int pd = model_->cfg().pos_dim, n2 = 2 * Tc - 1 + L;
    std::vector<float> pe((size_t)n2 * pd);
    const float cl = sqrtf((float)pd), ls = (float)pd / (2.0f * (float)M_PI), logcl = logf(cl);
    for (int n = 0; n < n2; n++) {
        float x = (float)(n - (Tc + L - 1));
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
    pe_cache_[key] = d;
    return d;
}

// Conv2dSubsampling.streaming_forward, NHWC.  x: [B,T,80] -> [B*Tc, D0]
float* Engine::encoder_embed_stream(const Ctx& c, const float* x, const int* d_slots, int B, int T, int* Tc_out) {
    const Model& m = *model_;
    const int F0 = 80, T1 = T - 2, T2 = (T1 - 3) / 2 + 1, F2 = (F0 - 3) / 2 + 1, T3 = T2 - 2, F3 = (F2 - 3) / 2 + 1, Tc = T3 - 3;
    K2_REQUIRE(Tc > 0 && F3 == 19, "streaming embed: chunk of %d frames unsupported", T);
    Arena& ar = *c.arena;
    const int D0 = m.cfg().dim[0];
    float* out = ar.take<float>((int64_t)B * Tc * D0);
    int64_t mark = ar.mark();
    float* a1 = ar.take<float>((int64_t)B * T1 * F0 * 8);
    conv0_swoosh(c, x, m.w("encoder_embed.conv.0.weight"), m.w("encoder_embed.conv.0.bias"), a1, B, T, F0);
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
    // ConvNeXt.streaming_forward: [cache(3) ; a3(T3)] -> valid 7-tap time conv -> Tc frames
    float* cat = ar.take<float>((int64_t)B * (T3 + 3) * F3 * 128);
    const int npix = B * Tc * F3;
    float* byp = ar.take<float>((int64_t)npix * 128);  // bypass = x[:, :, :Tc]
    convnext_cat(c, a3, online_pool_, lay_.floats_per_stream, lay_.embed, d_slots, cat, byp, B, T3, Tc, F3, 128);
    float* dw = ar.take<float>((int64_t)npix * 128);
    dwconv7x7(c, cat, m.w("encoder_embed.convnext.depthwise_conv.weight#kc"), m.w("encoder_embed.convnext.depthwise_conv.bias"), dw, B,
              T3 + 3, Tc, 0, F3, 128);
    float* hid = ar.take<float>((int64_t)npix * 384);
    linear(c, dw, 128, m.w("encoder_embed.convnext.pointwise_conv1.weight"), m.w("encoder_embed.convnext.pointwise_conv1.bias"), hid, 384,
           npix, 128, 384, ACT_SWOOSH_L);
    linear(c, hid, 384, m.w("encoder_embed.convnext.pointwise_conv2.weight"), m.w("encoder_embed.convnext.pointwise_conv2.bias"), byp, 128,
           npix, 384, 128, ACT_NONE, byp, 128);
    float* lin = ar.take<float>((int64_t)B * Tc * D0);
    linear(c, byp, F3 * 128, m.w("encoder_embed.out.weight#fc"), m.w("encoder_embed.out.bias"), lin, D0, B * Tc, F3 * 128, D0);
    biasnorm(c, lin, m.w("encoder_embed.out_norm.bias"), m.w("encoder_embed.out_norm.log_scale"), out, B * Tc, D0);
    ar.rewind(mark);
    *Tc_out = Tc;
    return out;
}

// The streaming Zipformer2 encoder of one (sub-)batch: x [B, T, feat] (log-floored) -> encoder_out [B*Tp, enc_dim]; caches of
// the B slots advanced in place (OnlineProjOfZipformer2.EncoderProj :491-618 without stack / unstack)
float* Engine::online_encoder_zip2(const Ctx& c, const float* d_x, const int* d_slots, const long long* d_plen, const int* d_chunks, int B) {
    const int Tp = online_frames_per_chunk();
    int Tc = 0;
    float* x = encoder_embed_stream(c, d_x, d_slots, B, model_->cfg().chunk_T, &Tc);
    K2_REQUIRE((Tc + 1) / 2 == Tp, "internal: chunk yields %d frames, expected %d", (Tc + 1) / 2, Tp);
    const StreamSite site{d_slots, d_plen, d_chunks};
    FullDimSegs segs;
    encoder_stacks(c, x, B, Tc, &site, -1, nullptr, nullptr, &segs);
    return encoder_head(c, segs, B, Tc, nullptr);
}

void Engine::online_step(const int* slots, const float* const* chunks, const long long* hyps, const long long* plens, const int* nchunks, int B,
                         int64_t* tokens, int32_t* ts, int32_t* n_tokens, const int* fifo_heads) {
    online_step_impl(slots, chunks, hyps, plens, nchunks, B, tokens, ts, n_tokens, fifo_heads, nullptr);
}
void Engine::online_step_beam(const int* slots, const float* const* chunks, const long long* plens, const int* nchunks, int B, int K,
                              const int* beam_in, int* beam_out, const int* fifo_heads) {
    K2_REQUIRE(K >= 1 && K <= kMaxBeam, "online beam search: beam %d out of range [1,%d]", K, kMaxBeam);
    K2_REQUIRE(!model_->cfg().ctc, "online beam search: a CTC model runs its own search");
    std::vector<long long> hyps(2 * (size_t)B, K2HIP_BLANK_ID);   // (the greedy search's context input; unused by the beam search)
    OnlineBeamIO io{K, beam_in, beam_out, nullptr};
    online_step_impl(slots, chunks, hyps.data(), plens, nchunks, B, nullptr, nullptr, nullptr, fifo_heads, &io);
}
void Engine::online_step_beam_hw(const int* slots, const float* const* chunks, const long long* plens, const int* nchunks, int B, int K,
                                 const int* beam_in, int* beam_out, const BeamHwIO& hw, const int* fifo_heads) {
    K2_REQUIRE(K >= 1 && K <= kMaxBeam, "online beam search: beam %d out of range [1,%d]", K, kMaxBeam);
    K2_REQUIRE(!model_->cfg().ctc, "online beam search: a CTC model runs its own search");
    std::vector<long long> hyps(2 * (size_t)B, K2HIP_BLANK_ID);
    OnlineBeamIO io{K, beam_in, beam_out, &hw};
    online_step_impl(slots, chunks, hyps.data(), plens, nchunks, B, nullptr, nullptr, nullptr, fifo_heads, &io);
}
void Engine::online_step_ctc_prefix(const int* slots, const float* const* chunks, const long long* plens, const int* nchunks, int B, int K,
                                    const int* cp_in, int* cp_out, const int* fifo_heads) {
    K2_REQUIRE(K >= 1 && K <= kMaxBeam, "online ctc prefix search: beam %d out of range [1,%d]", K, kMaxBeam);
    K2_REQUIRE(model_->cfg().ctc, "online ctc prefix search: the model has no CTC head");
    const CtcPrefixResumeLayout L{K, online_frames_per_chunk()};
    ctc_prefix_chunk_check_args(B, L.Tc, model_->cfg().V, nullptr, K, cp_in, L.in_ints(), L.in_e(), L.in_rel());
    std::vector<long long> hyps(2 * (size_t)B, K2HIP_BLANK_ID);   // (the greedy search's context input; unused here)
    OnlineCtcPrefixIO io{K, cp_in, cp_out};
    online_step_impl(slots, chunks, hyps.data(), plens, nchunks, B, nullptr, nullptr, nullptr, fifo_heads, nullptr, &io);
}
void Engine::online_step_ctc_prefix_bias(const int* slots, const float* const* chunks, const long long* plens, const int* nchunks, int B, int K,
                                         const int* cp_in, int* cp_out, const CtcPrefixBiasIO& bias, const int* fifo_heads) {
    K2_REQUIRE(K >= 1 && K <= kMaxBeam, "online ctc prefix search: beam %d out of range [1,%d]", K, kMaxBeam);
    K2_REQUIRE(model_->cfg().ctc, "online ctc prefix search: the model has no CTC head");
    K2_REQUIRE(bias.graphs && bias.side_in && bias.side_out, "online ctc prefix search: null side block");
    const CtcPrefixResumeLayout L{K, online_frames_per_chunk()};
    ctc_prefix_chunk_check_args(B, L.Tc, model_->cfg().V, nullptr, K, cp_in, L.in_ints(), L.in_e(), L.in_rel());
    std::vector<long long> hyps(2 * (size_t)B, K2HIP_BLANK_ID);
    OnlineCtcPrefixIO io{K, cp_in, cp_out, &bias};
    online_step_impl(slots, chunks, hyps.data(), plens, nchunks, B, nullptr, nullptr, nullptr, fifo_heads, nullptr, &io);
}
void Engine::online_step_impl(const int* slots, const float* const* chunks, const long long* hyps, const long long* plens, const int* nchunks,
                              int B, int64_t* tokens, int32_t* ts, int32_t* n_tokens, const int* fifo_heads, const OnlineBeamIO* beam,
                              const OnlineCtcPrefixIO* cpx) {
    online_ensure_pool();
    K2_REQUIRE(B > 0, "online_step: no ready stream");
    const Model& m = *model_;
    const Config& cf = m.cfg();
    const int T = cf.chunk_T, Tp = online_frames_per_chunk();
    SearchOut out;
    SearchExtras ex;
    // the streams' chunks, gathered once into pinned staging (one host copy; the H2D below is then a real asynchronous DMA)
    const size_t chunk_floats = (size_t)T * cf.feat;
    K2_HIP(hipSetDevice(device_));
    const bool from_fifo = fifo_heads != nullptr && online_fifo_ != nullptr;  // the chunks are already on the device (FIFO mirror)
    // ONE upload per tick: [chunks' frames (only when they are not on the device yet) | plens | hyps | slots | chunk counts | FIFO heads |
    // overflow flag = 0], packed in pinned staging in the device block's layout (five small copies from pageable memory + a memset were
    // six blit launches of ~4 us each at the head of the step); ONE download: the SearchOut block, whose flag is the upload's last 16 bytes
    // Under beam search the upload carries the streams' saved hypotheses and relation tables too (in front of the flag), and the
    // download is [flag | the surviving hypotheses' out blocks] instead of the greedy tokens.  With hotword graphs attached the saved
    // hypotheses' graph states and the streams' table pointers follow the in blocks, the survivors' states the out blocks.
    const BeamResumeLayout RL{beam ? beam->K : 1, Tp};
    const BeamHwIO* bhw = beam ? beam->hw : nullptr;
    // A CTC model under the carried prefix search: its in blocks ride where the beam search's do, its out blocks come back the same way
    // (the flag is the resumed kernel's status word)
    const CtcPrefixResumeLayout CL{cpx ? cpx->K : 1, Tp};
    K2_REQUIRE(!(beam && cpx), "internal: one search per tick");
    const int64_t nb_bin = beam ? (int64_t)sizeof(int) * RL.in_ints() * B : cpx ? (int64_t)sizeof(int) * CL.in_ints() * B : 0;
    // (a biased prefix search: its side in blocks and graph pointers ride where the beam search's states and graphs do, its side out
    // blocks behind the out blocks)
    const CtcPrefixBiasIO* cbias = cpx ? cpx->bias : nullptr;
    const CtcPrefixResumeBiasLayout CSL{cpx ? cpx->K : 1};
    const int64_t nb_cso = cbias ? (int64_t)sizeof(int) * CSL.out_ints() * B : 0;
    const int64_t nb_hst = bhw ? (int64_t)sizeof(int) * beam->K * B * bhw->planes() : cbias ? (int64_t)sizeof(int) * CSL.in_ints() * B : 0,
                  nb_hg = bhw || cbias ? (int64_t)sizeof(BeamHwStream) * B : 0;
    const int64_t nb_bout = beam ? (int64_t)sizeof(int) * RL.out_ints() * B + nb_hst : cpx ? (int64_t)sizeof(int) * CL.out_ints() * B + nb_cso : 0,
                  o_hout = nb_bout - (beam ? nb_hst : nb_cso);
    // (an active streaming neural LM fusion: the streams' block-pointer table rides behind the graphs, in the same upload)
    const NlmStreamIO* nlm_io = beam ? nlm_io_host_ : nullptr;
    K2_REQUIRE(!nlm_io || rnn_lm_stream_fusion_active(), "online beam search: state blocks without an active streaming neural LM fusion");
    const int64_t nb_nl = nlm_io ? (int64_t)sizeof(NlmStreamIO) * B : 0;
    const int64_t nb_x = from_fifo ? 0 : (int64_t)sizeof(float) * chunk_floats * B;
    const int64_t o_plen = align_up(nb_x, 16), o_hyp = o_plen + 8 * (int64_t)B, o_slots = o_hyp + 16 * (int64_t)B, o_chunks = o_slots + 4 * (int64_t)B,
                  o_heads = o_chunks + 4 * (int64_t)B, o_bin = align_up(o_heads + 4 * (int64_t)B, 16), o_hst = align_up(o_bin + nb_bin, 16),
                  o_hg = align_up(o_hst + nb_hst, 16), o_nl = align_up(o_hg + nb_hg, 16), o_ovf = align_up(o_nl + nb_nl, 16), in_bytes = o_ovf + 16;
    char* stage = static_cast<char*>(pinned_in(in_bytes));
    if (!from_fifo)
        for (int b = 0; b < B; b++) memcpy(stage + (size_t)b * chunk_floats * sizeof(float), chunks[b], sizeof(float) * chunk_floats);
    memcpy(stage + o_plen, plens, sizeof(long long) * B);
    memcpy(stage + o_hyp, hyps, sizeof(long long) * 2 * B);
    memcpy(stage + o_slots, slots, sizeof(int) * B);
    memcpy(stage + o_chunks, nchunks, sizeof(int) * B);
    if (from_fifo) memcpy(stage + o_heads, fifo_heads, sizeof(int) * B);
    else memset(stage + o_heads, 0, sizeof(int) * B);
    if (beam) memcpy(stage + o_bin, beam->in, (size_t)nb_bin);
    if (cpx) memcpy(stage + o_bin, cpx->in, (size_t)nb_bin);
    if (bhw) {
        memcpy(stage + o_hst, bhw->st_in, (size_t)nb_hst);
        memcpy(stage + o_hg, bhw->graphs, (size_t)nb_hg);
    }
    if (cbias) {
        memcpy(stage + o_hst, cbias->side_in, (size_t)nb_hst);
        memcpy(stage + o_hg, cbias->graphs, (size_t)nb_hg);
    }
    if (nlm_io) memcpy(stage + o_nl, nlm_io, (size_t)nb_nl);
    memset(stage + o_ovf, 0, 16);
    const int64_t nb_out = beam || cpx ? nb_bout : SearchOut::bytes_for(B, Tp) - 16;   // what follows the flag
    run_sized([&](const Ctx& c) {
        Arena& ar = *c.arena;
        // one device block: the inputs, the overflow flag (uploaded as zero: the last 16 bytes of the input part), the outputs right
        // behind it -- a SearchOut placed on the flag, or under beam search [flag | out blocks]
        char* d_in = ar.take<char>(in_bytes + nb_out);
        char* d_out = d_in + in_bytes;
        out = SearchOut(d_in + o_ovf, B, Tp);
        float* d_x = from_fifo ? ar.take<float>((int64_t)B * T * cf.feat) : reinterpret_cast<float*>(d_in);
        long long* d_plen = reinterpret_cast<long long*>(d_in + o_plen);
        long long* d_hyp = reinterpret_cast<long long*>(d_in + o_hyp);
        int* d_slots = reinterpret_cast<int*>(d_in + o_slots);
        int* d_chunks = reinterpret_cast<int*>(d_in + o_chunks);
        int* d_heads = reinterpret_cast<int*>(d_in + o_heads);
        const BeamHwIO dhw{reinterpret_cast<const BeamHwStream*>(d_in + o_hg), reinterpret_cast<const int*>(d_in + o_hst),
                           reinterpret_cast<int*>(d_out + o_hout), bhw && bhw->lm, bhw && bhw->lodr};
        if (!c.dry) {
            K2_HIP(hipEventRecord(ev_[0], c.stream));
            K2_HIP(hipMemcpyAsync(d_in, stage, (size_t)in_bytes, hipMemcpyHostToDevice, c.stream));
        }
        // online PadSequence (PadHelper.cs:9-13,58): the floor of genuine zeros runs inside the gather when the chunks come from the FIFO
        if (from_fifo) fifo_gather(c, online_fifo_, kFifoFrames, cf.feat, d_slots, d_heads, d_x, B, T);
        else logfloor_inplace(c, d_x, (long long)B * T * cf.feat);
        float* enc = nullptr;
        if (cf.lstm || cf.conformer || cf.zip1) {
            int tc = Tp;
            enc = cf.lstm ? lstm_chunk(c, d_x, d_slots, B) : cf.zip1 ? zip1_chunk(c, d_x, d_slots, B, &tc) : conformer_chunk(c, d_x, d_slots, d_plen, B, &tc);
            K2_REQUIRE(tc == Tp, "internal: chunk yields %d frames, expected %d", tc, Tp);
        } else {
            enc = online_encoder_zip2(c, d_x, d_slots, d_plen, d_chunks, B);
        }
        if (!c.dry) K2_HIP(hipEventRecord(ev_[3], c.stream));
        if (cf.ctc) {
            // OnlineRecognizer.ForwardBatchGreedySearchCTC (:220-313): per-chunk CTC collapse, prev_id reset per chunk
            // ... or, for streams that opted in, the prefix search resumed from their carried prefixes on the tick's log-probs
            if (cpx) {
                CtcPrefixResumeBiasArgs a;
                a.log_probs = enc; a.B = B; a.Tc = Tp; a.V = cf.V; a.beam = cpx->K;
                a.nodes = ar.take<int4>((int64_t)B * Tp * cpx->K);
                a.in = reinterpret_cast<const int*>(d_in + o_bin);
                a.out = reinterpret_cast<int*>(d_out);
                a.status = out.flag();
                if (cbias) {
                    a.hw_streams = reinterpret_cast<const BeamHwStream*>(d_in + o_hg);
                    a.side_in = reinterpret_cast<const int*>(d_in + o_hst);
                    a.side_out = reinterpret_cast<int*>(d_out + o_hout);
                    if (cbias->lm) a.lm = lm_;
                    ctc_prefix_resume_biased(c, a);
                } else {
                    ctc_prefix_resume(c, a);   // (no stream of the tick is biased: the plain launch, unchanged)
                }
            } else {
                ex = ctc_device(c, enc, B, Tp, out);
            }
        } else if (beam) {   // modified beam search resumed from the streams' saved hypotheses, on the tick's encoder buffer
            beam_resume_device(c, enc, B, Tp, beam->K, reinterpret_cast<const int*>(d_in + o_bin), reinterpret_cast<int*>(d_out), out.flag(),
                               bhw ? &dhw : nullptr, nlm_io ? reinterpret_cast<const NlmStreamIO*>(d_in + o_nl) : nullptr);
        } else {
            // OnlineRecognizer.cs:135-202: decoder on the streams' hyps, T' joiner steps, skip {blank, unk, 1}
            GreedyArgs a;
            a.enc = enc; a.B = B; a.Tp = Tp; a.t0 = nullptr; a.skip1 = 1; a.max_sym = INT_MAX;
            a.tokens = out.tokens(); a.timestamps = out.timestamps(); a.n_tokens = out.counts(); a.max_tokens = Tp; a.overflow = out.flag();
            a.init_ctx = d_hyp; a.screen_counts = screen_counts();
            // rounds of joiner GEMMs + a per-stream step kernel, or the persistent kernel where its rounds go through the f16 screen
            // (measured per model: greedy_loop_screens)
            const bool persistent_search = tunables().search_rounds == 0 || (tunables().search_rounds < 0 && greedy_loop_screens(decjoin(), B, true, c.one_part));
            if (persistent_search) greedy_loop(c, decjoin(), a);
            else greedy_rounds(c, decjoin(), model_->w("joiner.output_linear.weight"), a);
        }
        if (!c.dry) K2_HIP(hipEventRecord(ev_[4], c.stream));
    });
    if (cpx) {   // ONE download: [status | out blocks]
        char* pin = static_cast<char*>(pinned(16 + nb_bout));
        K2_HIP(hipMemcpyAsync(pin, out.flag(), (size_t)(16 + nb_bout), hipMemcpyDeviceToHost, stream_));
        K2_HIP(hipEventRecord(ev_[5], stream_));
        K2_HIP(hipStreamSynchronize(stream_));
        if (*reinterpret_cast<int*>(pin)) failf(K2HIP_ERR_HIP, "online ctc prefix search: an in block contradicts itself");
        memcpy(cpx->out, pin + 16, (size_t)o_hout);
        if (cbias) memcpy(cbias->side_out, pin + 16 + o_hout, (size_t)nb_cso);
    } else if (beam) {   // ONE download: [flag | out blocks]
        char* pin = static_cast<char*>(pinned(16 + nb_bout));
        K2_HIP(hipMemcpyAsync(pin, out.flag(), (size_t)(16 + nb_bout), hipMemcpyDeviceToHost, stream_));
        K2_HIP(hipEventRecord(ev_[5], stream_));
        K2_HIP(hipStreamSynchronize(stream_));
        if (*reinterpret_cast<int*>(pin)) failf(K2HIP_ERR_HIP, "online beam search: a hypothesis outgrew its buffer");
        memcpy(beam->out, pin + 16, (size_t)o_hout);
        if (bhw) memcpy(bhw->st_out, pin + 16 + o_hout, (size_t)nb_hst);
        fetch_beam_yp();
    } else {
        finish_tokens(out, ex, tokens, ts, n_tokens);
    }
    fill_timing(false, false);
}

// IOnlineProj.EncoderProj (OnlineProjOfZipformer2.cs:491-618) as an operator: feats [B, chunk_T, feat] host, the B slots' caches
// advance in place, encoder_out [B, T', joiner_dim] to host.  The search is the caller's (DecoderProj / JoinerProj).  A streaming
// zipformer2ctc model delivers [B, T', V] log-probs instead (encoder_head ends in the CTC head and the row log-softmax): the producer of
// k2hip_ctc_prefix_beam_search_chunk.
void Engine::online_encoder(const int* slots, const float* feats, const long long* plens, const int* nchunks, int B, float* enc_out) {
    online_ensure_pool();
    K2_REQUIRE(B > 0, "online_encoder: empty batch");
    const Config& cf = model_->cfg();
    K2_REQUIRE(cf.streaming && !cf.lstm && !cf.conformer && !cf.zip1, "online_encoder: streaming Zipformer2 models only");
    const int T = cf.chunk_T, Tp = online_frames_per_chunk();
    K2_HIP(hipSetDevice(device_));
    const size_t in_bytes = sizeof(float) * (size_t)B * T * cf.feat;
    float* stage = static_cast<float*>(pinned_in((int64_t)in_bytes));
    memcpy(stage, feats, in_bytes);
    float* d_enc = nullptr;
    run_sized([&](const Ctx& c) {
        Arena& ar = *c.arena;
        float* d_x = ar.take<float>((int64_t)B * T * cf.feat);
        int* d_slots = ar.take<int>(B);
        long long* d_plen = ar.take<long long>(B);
        int* d_chunks = ar.take<int>(B);
        if (!c.dry) {
            K2_HIP(hipMemcpyAsync(d_x, stage, in_bytes, hipMemcpyHostToDevice, c.stream));
            K2_HIP(hipMemcpyAsync(d_slots, slots, sizeof(int) * B, hipMemcpyHostToDevice, c.stream));
            K2_HIP(hipMemcpyAsync(d_chunks, nchunks, sizeof(int) * B, hipMemcpyHostToDevice, c.stream));
            K2_HIP(hipMemcpyAsync(d_plen, plens, sizeof(long long) * B, hipMemcpyHostToDevice, c.stream));
        }
        logfloor_inplace(c, d_x, (long long)B * T * cf.feat);
        d_enc = online_encoder_zip2(c, d_x, d_slots, d_plen, d_chunks, B);
    });
    K2_HIP(hipMemcpyAsync(enc_out, d_enc, sizeof(float) * (size_t)B * Tp * cf.enc_dim(), hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
}

}  // namespace k2hip
