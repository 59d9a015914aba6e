// Engine: voice activity detection and long recordings (DESIGN.md "Voice activity detection and long recordings").  The host side of
// vad.hip: the call's descriptors and carried blocks laid out and checked before any device work, one upload, the launches, one
// download; and the long entry: resident features, the detector, the segments packed into batches and decoded by the offline path's
// own tail (pad_logfloor reads each segment's rows out of the resident block: the device-to-device gather).
#include <chrono>

#include "engine.h"

namespace k2hip {

void Engine::vad_device_call(VadJob* jobs, int B, const std::function<void(const Ctx&, std::vector<const float*>&)>& prepare) {
    const int F = model_->cfg().feat;
    // the active streams, their descriptors (feats filled in later) and carried blocks
    std::vector<int> act;
    std::vector<VadRow> rows;
    long long n_work = 0, n_state = 0, n_segs = 0;
    for (int b = 0; b < B; b++) {
        const VadJob& j = jobs[b];
        K2_REQUIRE(j.cfg && j.st && j.segs && j.n >= 0, "vad: stream %d: bad arguments", b);
        if (j.n == 0) continue;
        const k2hip_vad_config& c = *j.cfg;
        vad_check_config(c, F);
        const VadState& st = *j.st;
        K2_REQUIRE(st.frames >= 0 && st.frames + j.n < kVadMaxFrames, "vad: stream %d: %lld + %lld frames between resets (at most 2^30)", b,
                   (long long)st.frames, (long long)j.n);
        K2_REQUIRE((int64_t)st.m.size() == std::min<int64_t>(st.frames, c.floor_window - 1), "vad: stream %d carries %zu values of m at frame %lld", b,
                   st.m.size(), (long long)st.frames);
        VadRow r;
        r.stride = F;
        r.n = (int)j.n; r.t0 = (int)st.frames; r.n_hist = (int)st.m.size();
        r.lo = c.band_lo; r.hi = c.band_hi; r.W = c.floor_window;
        r.inv_band = 1.0f / (float)(c.band_hi - c.band_lo);
        r.rise = c.rise; r.margin = c.margin; r.abs_floor = c.abs_floor;
        r.min_silence = c.min_silence; r.min_speech = c.min_speech; r.max_speech = c.max_speech;
        r.trig = st.trig; r.start = (int)st.start; r.te = (int)st.te;
        r.work_off = n_work; r.state_off = n_state; r.seg_off = n_segs;
        // forced cuts are at least max_speech / 2 >= min_speech frames apart, unforced ends at least min_speech + min_silence (an unforced
        // end may follow a forced cut closely: a pause that was running when the cut fell well before it)
        r.seg_cap = (int)(2 * (j.n / c.min_speech) + 4);
        n_work += j.n;
        n_state += vad_state_words(c.floor_window);
        n_segs += r.seg_cap;
        act.push_back(b);
        rows.push_back(r);
    }
    vad_taps_ = VadTaps();
    vad_taps_.off.assign((size_t)B + 1, 0);
    if (act.empty()) return;
    const int A = (int)act.size();
    const int64_t nb_rows = align_up((int64_t)sizeof(VadRow) * A, 16), nb_state = align_up(4 * n_state, 16);
    // the download: [new blocks | segments | m | n | d]
    const int64_t o_seg = nb_state, o_m = o_seg + align_up(12 * n_segs, 16), o_n = o_m + align_up(4 * n_work, 16), o_d = o_n + align_up(4 * n_work, 16);
    const int64_t nb_down = o_d + align_up(n_work, 16);
    char* pin_up = static_cast<char*>(pinned_in(nb_rows + nb_state + 64));
    char* pin_down = static_cast<char*>(pinned(nb_down + 64));
    VadRow* h_rows = reinterpret_cast<VadRow*>(pin_up);
    float* h_state = reinterpret_cast<float*>(pin_up + nb_rows);
    memset(h_state, 0, (size_t)nb_state);
    for (int a = 0; a < A; a++) {
        const VadState& st = *jobs[act[(size_t)a]].st;
        const int W = rows[(size_t)a].W;
        float* blk = h_state + rows[(size_t)a].state_off;
        if (!st.m.empty()) memcpy(blk + (W - 1) - st.m.size(), st.m.data(), sizeof(float) * st.m.size());
        memcpy(blk + (W - 1), st.s, sizeof(float) * 4);
    }
    char* d_down = nullptr;
    std::vector<const float*> d_feats((size_t)B, nullptr);
    run_sized([&](const Ctx& c) {
        prepare(c, d_feats);
        char* d_up = c.arena->take<char>(nb_rows + nb_state);
        d_down = c.arena->take<char>(nb_down);
        float* d_s = c.arena->take<float>(n_work);
        for (int a = 0; a < A; a++) {   // (the rows name device addresses: the same in both passes once the arena is sized)
            rows[(size_t)a].feats = d_feats[(size_t)act[(size_t)a]];
            h_rows[a] = rows[(size_t)a];
        }
        if (!c.dry) K2_HIP(hipMemcpyAsync(d_up, pin_up, (size_t)(nb_rows + nb_state), hipMemcpyHostToDevice, c.stream));
        VadBuffers buf;
        buf.st_in = reinterpret_cast<const float*>(d_up + nb_rows);
        buf.st_out = reinterpret_cast<float*>(d_down);
        buf.s = d_s;
        buf.m = reinterpret_cast<float*>(d_down + o_m);
        buf.n = reinterpret_cast<float*>(d_down + o_n);
        buf.d = reinterpret_cast<unsigned char*>(d_down + o_d);
        buf.segs = reinterpret_cast<int*>(d_down + o_seg);
        buf.n_work = n_work; buf.n_state = n_state; buf.n_segs = n_segs;
        vad_run(c, rows.data(), reinterpret_cast<const VadRow*>(d_up), A, buf);
    });
    K2_HIP(hipMemcpyAsync(pin_down, d_down, (size_t)nb_down, hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
    // nothing of any stream has moved so far; check the whole download before the first state changes
    const float* o_state = reinterpret_cast<const float*>(pin_down);
    const int* o_segs = reinterpret_cast<const int*>(pin_down + o_seg);
    for (int a = 0; a < A; a++) {
        const VadRow& r = rows[(size_t)a];
        const int* mi = reinterpret_cast<const int*>(o_state + r.state_off + r.W + 3);
        K2_REQUIRE(mi[3] >= 0 && mi[3] <= r.seg_cap, "internal: the detector emitted %d segments for stream %d, room for %d", mi[3], act[(size_t)a], r.seg_cap);
    }
    vad_taps_.m.assign(reinterpret_cast<const float*>(pin_down + o_m), reinterpret_cast<const float*>(pin_down + o_m) + n_work);
    vad_taps_.n.assign(reinterpret_cast<const float*>(pin_down + o_n), reinterpret_cast<const float*>(pin_down + o_n) + n_work);
    vad_taps_.d.assign(reinterpret_cast<const uint8_t*>(pin_down + o_d), reinterpret_cast<const uint8_t*>(pin_down + o_d) + n_work);
    for (int a = 0, b = 0; b <= B; b++) {
        vad_taps_.off[(size_t)b] = a < A ? rows[(size_t)a].work_off : n_work;
        if (a < A && act[(size_t)a] == b) a++;
    }
    for (int a = 0; a < A; a++) {
        const VadRow& r = rows[(size_t)a];
        VadJob& j = jobs[act[(size_t)a]];
        VadState& st = *j.st;
        const float* blk = o_state + r.state_off;
        const int* mi = reinterpret_cast<const int*>(blk + r.W + 3);
        st.frames += j.n;
        const size_t keep = (size_t)std::min<int64_t>(st.frames, r.W - 1);
        st.m.assign(blk + (r.W - 1) - keep, blk + (r.W - 1));
        memcpy(st.s, blk + (r.W - 1), sizeof(float) * 4);
        st.trig = mi[0]; st.start = mi[1]; st.te = mi[2];
        for (int k = 0; k < mi[3]; k++) {
            const int* g = o_segs + 3 * (r.seg_off + k);
            j.segs->push_back(vad_report(*j.cfg, VadRaw{g[0], g[1], g[2]}, &st.prev_end, st.frames));
        }
    }
}

void Engine::vad_host(VadJob* jobs, int B, bool from_samples) {
    K2_REQUIRE(jobs && B > 0, "vad: empty call");
    K2_HIP(hipSetDevice(device_));
    if (fb_pending_.active) fbank_gather_finish();   // (the staging buffer below is the deferred fbank gather's: one user at a time)
    const int F = model_->cfg().feat;
    if (!from_samples) {
        int64_t total = 0;
        for (int b = 0; b < B; b++) {
            K2_REQUIRE(jobs[b].n >= 0 && (jobs[b].n == 0 || jobs[b].feats), "vad: stream %d has no features", b);
            total += jobs[b].n;
        }
        // the rows of all streams back to back in one pinned block -> one upload
        float* pin = static_cast<float*>(pinned_fb((int64_t)sizeof(float) * total * F + 64));
        int64_t o = 0;
        std::vector<int64_t> off((size_t)B);
        for (int b = 0; b < B; b++) {
            off[(size_t)b] = o;
            if (jobs[b].n) memcpy(pin + o, jobs[b].feats, sizeof(float) * (size_t)jobs[b].n * F);
            o += jobs[b].n * F;
        }
        vad_device_call(jobs, B, [&](const Ctx& c, std::vector<const float*>& d_feats) {
            float* d_x = c.arena->take<float>(total * F);
            if (!c.dry && total) K2_HIP(hipMemcpyAsync(d_x, pin, sizeof(float) * (size_t)total * F, hipMemcpyHostToDevice, c.stream));
            for (int b = 0; b < B; b++) d_feats[(size_t)b] = d_x + off[(size_t)b];
        });
        return;
    }
    // samples: [head ; tail] of every stream that gives a frame as rows of one dense block (tails zeroed: a kept frame never reads them),
    // ONE batched fbank launch, the detector on its output
    int64_t nmax = 0;
    int G = 0;
    std::vector<int> row_of((size_t)B, -1);
    for (int b = 0; b < B; b++) {
        VadJob& j = jobs[b];
        K2_REQUIRE(j.n_head >= 0 && j.n_tail >= 0 && (j.n_head == 0 || j.head) && (j.n_tail == 0 || j.tail), "vad: stream %d: bad samples", b);
        j.n = fbank_num_frames(j.n_head + j.n_tail);
        if (j.n == 0) continue;
        row_of[(size_t)b] = G++;
        nmax = std::max(nmax, j.n_head + j.n_tail);
    }
    if (G == 0) return vad_device_call(jobs, B, [](const Ctx&, std::vector<const float*>&) {});
    const int64_t ns = (nmax + 3) & ~(int64_t)3, nf = fbank_num_frames(nmax);
    float* pin = static_cast<float*>(pinned_fb((int64_t)sizeof(float) * G * ns + 64));
    for (int b = 0; b < B; b++) {
        if (row_of[(size_t)b] < 0) continue;
        const VadJob& j = jobs[b];
        float* row = pin + (size_t)row_of[(size_t)b] * ns;
        if (j.n_head) memcpy(row, j.head, sizeof(float) * (size_t)j.n_head);
        if (j.n_tail) memcpy(row + j.n_head, j.tail, sizeof(float) * (size_t)j.n_tail);
        const int64_t have = j.n_head + j.n_tail;
        if (have < ns) memset(row + have, 0, sizeof(float) * (size_t)(ns - have));
    }
    vad_device_call(jobs, B, [&](const Ctx& c, std::vector<const float*>& d_feats) {
        float* d_s = c.arena->take<float>((int64_t)G * ns);
        float* d_x = c.arena->take<float>((int64_t)G * nf * F);
        if (!c.dry) K2_HIP(hipMemcpyAsync(d_s, pin, sizeof(float) * (size_t)G * ns, hipMemcpyHostToDevice, c.stream));
        fbank(c, fbank_args(d_s, nmax, ns, G, nf, d_x));
        for (int b = 0; b < B; b++)
            if (row_of[(size_t)b] >= 0) d_feats[(size_t)b] = d_x + (int64_t)row_of[(size_t)b] * nf * F;
    });
}

namespace {
struct DevBlock {   // a device allocation for the length of one call
    void* p = nullptr;
    ~DevBlock() {
        if (p) (void)hipFree(p);
    }
};
double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
}  // namespace

void Engine::recognize_long(const float* samples, int64_t n, const k2hip_vad_config& cfg, int max_batch, int64_t max_batch_frames,
                            std::vector<LongSegment>* out) {
    const Config& cf = model_->cfg();
    const int F = cf.feat;
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
    K2_HIP(hipSetDevice(device_));
    // ---- fbank over the whole recording into a resident [T][F] block
    auto t0 = std::chrono::steady_clock::now();
    DevBlock feats, wav;
    K2_HIP(hipMalloc(&feats.p, sizeof(float) * (size_t)T * F));
    K2_HIP(hipMalloc(&wav.p, sizeof(float) * (size_t)n));
    K2_HIP(hipMemcpyAsync(wav.p, samples, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, stream_));
    float* d_feats = static_cast<float*>(feats.p);
    run_sized([&](const Ctx& c) { fbank(c, fbank_args(static_cast<const float*>(wav.p), n, n, 1, T, d_feats)); });
    K2_HIP(hipStreamSynchronize(stream_));
    K2_HIP(hipFree(wav.p));
    wav.p = nullptr;
    long_ms_[0] = ms_since(t0);
    // ---- the detector over all frames, then its flush
    t0 = std::chrono::steady_clock::now();
    VadState st;
    std::vector<VadSeg> segs;
    VadJob job;
    job.cfg = &cfg; job.st = &st; job.n = T; job.segs = &segs;
    vad_device_call(&job, 1, [&](const Ctx&, std::vector<const float*>& d) { d[0] = d_feats; });
    vad_ref_flush(cfg, st, &segs);
    long_ms_[1] = ms_since(t0);
    // ---- the segments, in order, in batches
    t0 = std::chrono::steady_clock::now();
    const int S = (int)segs.size();
    std::vector<int64_t> len((size_t)S);
    for (int i = 0; i < S; i++) len[(size_t)i] = segs[(size_t)i].end - segs[(size_t)i].start;
    std::vector<int32_t> batch_of;
    vad_pack_batches(len.data(), S, max_batch, max_batch_frames, &batch_of);
    out->resize((size_t)S);
    for (int i0 = 0; i0 < S;) {
        int i1 = i0;
        int64_t longest = 0;
        while (i1 < S && batch_of[(size_t)i1] == batch_of[(size_t)i0]) longest = std::max(longest, len[(size_t)i1++]);
        const int B = i1 - i0;
        const OfflineShape sh = offline_shape("recognize_long", longest * F, true);
        const int max_tokens = std::max(1, sh.Tp);
        std::vector<long long> off((size_t)B), ln((size_t)B);
        for (int b = 0; b < B; b++) {
            off[(size_t)b] = (long long)segs[(size_t)(i0 + b)].start * F;
            ln[(size_t)b] = (long long)len[(size_t)(i0 + b)] * F;
        }
        char* pin = static_cast<char*>(pinned(std::max<int64_t>(16 * (int64_t)B, SearchOut::bytes_for(B, max_tokens)) + 64));
        memcpy(pin, off.data(), sizeof(long long) * (size_t)B);
        memcpy(pin + 8 * (size_t)B, ln.data(), sizeof(long long) * (size_t)B);
        SearchOut so;
        SearchExtras ex;
        SearchStage stage;
        stage.keep_nbest = false;   // the best hypothesis only
        run_sized([&](const Ctx& c) {
            Arena& ar = *c.arena;
            so = SearchOut(ar, B, max_tokens);
            long long* d_off = ar.take<long long>(2 * B);
            float* d_x = ar.take<float>((int64_t)B * sh.L);
            if (!c.dry) {
                K2_HIP(hipEventRecord(ev_[0], c.stream));
                K2_HIP(hipMemcpyAsync(d_off, pin, 16 * (size_t)B, hipMemcpyHostToDevice, c.stream));
                K2_HIP(hipEventRecord(ev_[1], c.stream));
            }
            pad_logfloor(c, d_feats, d_off, d_off + B, d_x, B, sh.L);   // each segment's rows out of the resident block
            ex = encode_and_search(c, d_x, B, sh.T, stage, so);
        });
        std::vector<int64_t> tok((size_t)B * max_tokens);
        std::vector<int32_t> ts((size_t)B * max_tokens), nt((size_t)B);
        finish_tokens(so, ex, tok.data(), ts.data(), nt.data());
        fill_timing(false, true);
        for (int b = 0; b < B; b++) {
            LongSegment& g = (*out)[(size_t)(i0 + b)];
            const VadSeg& v = segs[(size_t)(i0 + b)];
            g.start = v.start; g.end = v.end; g.forced = v.forced; g.batch = batch_of[(size_t)(i0 + b)];
            g.tokens.assign(tok.begin() + (size_t)b * max_tokens, tok.begin() + (size_t)b * max_tokens + nt[(size_t)b]);
            g.timestamps.assign(ts.begin() + (size_t)b * max_tokens, ts.begin() + (size_t)b * max_tokens + nt[(size_t)b]);
        }
        i0 = i1;
    }
    long_ms_[2] = ms_since(t0);
}

}  // namespace k2hip
