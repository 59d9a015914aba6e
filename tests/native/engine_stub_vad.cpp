// CPU stand-in of the engine's voice activity entries (Engine::vad_host, Engine::recognize_long) for the sanitizer builds of the host
// layer: the float32 host reference of csrc/vad_ref.h where the engine launches the kernels, over exact-size copies of the inputs (a
// read past a stream's rows or samples is a heap overflow the sanitizer sees), with the extents the real engine checks on the host
// checked here too, so that the stream bookkeeping of api.cpp -- remainders, the resampler's carried input, segments, the result
// object of the long entry -- runs unmodified.  The fake fbank gives every bin of frame t the value of the frame's first sample, so
// that a driver steers the detector through the samples; the fake search emits token 3 + (frames % 5) on every third encoder frame.
// Never linked into libk2hip.so.
#include <vector>

#include "../../k2transducerasr_amd/csrc/engine.h"
#include "../../k2transducerasr_amd/csrc/vad_ref.h"

namespace k2hip {

namespace {
std::vector<float> fake_fbank(const float* head, int64_t n_head, const float* tail, int64_t n_tail, const FbankOpts& f, int feat, int64_t nf) {
    std::vector<float> cat;
    cat.reserve((size_t)(n_head + n_tail));
    if (n_head) cat.insert(cat.end(), head, head + n_head);
    if (n_tail) cat.insert(cat.end(), tail, tail + n_tail);
    std::vector<float> out((size_t)nf * feat);
    for (int64_t t = 0; t < nf; t++) {
        volatile float last = cat[(size_t)(t * f.frame_shift + f.frame_len - 1)];   // (the whole frame must be there)
        (void)last;
        for (int c = 0; c < feat; c++) out[(size_t)(t * feat + c)] = cat[(size_t)(t * f.frame_shift)];
    }
    return out;
}
}  // namespace

void Engine::vad_host(VadJob* jobs, int B, bool from_samples) {
    K2_REQUIRE(jobs && B > 0, "vad: empty call");
    const int F = model_->cfg().feat;
    vad_taps_ = VadTaps();
    vad_taps_.off.assign((size_t)B + 1, 0);
    // everything is checked, and the new states are worked out on copies, before the first stream moves
    std::vector<VadState> next((size_t)B);
    std::vector<std::vector<VadSeg>> found((size_t)B);
    for (int b = 0; b < B; b++) {
        VadJob& j = jobs[b];
        K2_REQUIRE(j.cfg && j.st && j.segs, "vad: stream %d: bad arguments", b);
        std::vector<float> rows;
        if (from_samples) {
            K2_REQUIRE(j.n_head >= 0 && j.n_tail >= 0 && (j.n_head == 0 || j.head) && (j.n_tail == 0 || j.tail), "vad: stream %d: bad samples", b);
            j.n = fbank_num_frames(j.n_head + j.n_tail);
            rows = fake_fbank(j.head, j.n_head, j.tail, j.n_tail, model_->cfg().fbank, F, j.n);
        } else {
            K2_REQUIRE(j.n >= 0 && (j.n == 0 || j.feats), "vad: stream %d has no features", b);
            if (j.n) rows.assign(j.feats, j.feats + j.n * F);
        }
        vad_taps_.off[(size_t)b + 1] = vad_taps_.off[(size_t)b] + j.n;
        if (j.n == 0) continue;
        vad_check_config(*j.cfg, F);
        K2_REQUIRE((int64_t)j.st->m.size() == std::min<int64_t>(j.st->frames, j.cfg->floor_window - 1), "vad: stream %d carries %zu values of m at frame %lld",
                   b, j.st->m.size(), (long long)j.st->frames);
        next[(size_t)b] = *j.st;
        const size_t o = vad_taps_.m.size();
        vad_taps_.m.resize(o + (size_t)j.n);
        vad_taps_.n.resize(o + (size_t)j.n);
        vad_taps_.d.resize(o + (size_t)j.n);
        vad_ref_push(*j.cfg, next[(size_t)b], rows.data(), j.n, F, &found[(size_t)b], vad_taps_.m.data() + o, vad_taps_.n.data() + o, vad_taps_.d.data() + o);
    }
    for (int b = 0; b < B; b++) {
        if (jobs[b].n == 0) continue;
        *jobs[b].st = std::move(next[(size_t)b]);
        jobs[b].segs->insert(jobs[b].segs->end(), found[(size_t)b].begin(), found[(size_t)b].end());
    }
}

void Engine::recognize_long(const float* samples, int64_t n, const k2hip_vad_config& cfg, int max_batch, int64_t max_batch_frames,
                            std::vector<LongSegment>* out) {
    const int F = model_->cfg().feat;
    K2_REQUIRE(samples && out && n > 0, "recognize_long: no samples");
    K2_REQUIRE(max_batch > 0 && max_batch_frames > 0, "recognize_long: max_batch = %d, max_batch_frames = %lld", max_batch, (long long)max_batch_frames);
    vad_check_config(cfg, F);
    if (n > kLongMaxSamples)
        failf(K2HIP_ERR_UNSUPPORTED, "recognize_long: %lld samples at the model's rate exceed the limit of %lld (split the recording)", (long long)n,
              (long long)kLongMaxSamples);
    out->clear();
    long_ms_ = {0, 0, 0};
    const int64_t T = fbank_num_frames(n);
    if (T == 0) return;
    const std::vector<float> rows = fake_fbank(samples, n, nullptr, 0, model_->cfg().fbank, F, T);
    VadState st;
    std::vector<VadSeg> segs;
    vad_ref_push(cfg, st, rows.data(), T, F, &segs, nullptr, nullptr, nullptr);
    vad_ref_flush(cfg, st, &segs);
    std::vector<int64_t> len(segs.size());
    for (size_t i = 0; i < segs.size(); i++) len[i] = segs[i].end - segs[i].start;
    std::vector<int32_t> batch_of;
    vad_pack_batches(len.data(), (int)segs.size(), max_batch, max_batch_frames, &batch_of);
    out->resize(segs.size());
    for (size_t i = 0; i < segs.size(); i++) {
        LongSegment& g = (*out)[i];
        g.start = segs[i].start; g.end = segs[i].end; g.forced = segs[i].forced; g.batch = batch_of[i];
        int64_t longest = 0;   // T' comes from the longest segment of the batch, as the padded batch's does
        for (size_t k = 0; k < segs.size(); k++)
            if (batch_of[k] == batch_of[i]) longest = std::max(longest, len[k]);
        const int Tp = encoder_out_frames((int)longest + 19);
        for (int t = 0; t < std::min<int64_t>(Tp, (len[i] + 3) / 4); t += 3) {
            g.tokens.push_back(3 + len[i] % 5);
            g.timestamps.push_back(t);
        }
    }
}

}  // namespace k2hip
