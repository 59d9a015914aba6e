// Neural LM rescoring on the gfx950 kernels (rnn_lm.hip): the LM's upload and the scoring call over the rows of rnn_lm_plan.h.
//
// Per layer the input products of ALL rows of a time block are one MFMA GEMM through the project's launcher ([rows, in] x [in, 4H],
// bias in its epilogue); the recurrence is one rnn_lm_step launch per position, which reads step t - 1's rows of the layer's output as
// its A operand and writes step t's.  The last layer's rows go through rnn_lm_score_rows (no logits in memory) and rnn_lm_totals.
#include <cmath>

#include "engine.h"

namespace k2hip {

void* Engine::rnn_lm_upload(const RnnLm& m, RnnLmDev* out) {
    K2_HIP(hipSetDevice(device_));
    const int V = m.V, E = m.E, H = m.H, L = m.L, Vp = (V + 31) / 32 * 32;
    K2_REQUIRE(L >= 1 && L <= kRnnLmMaxLayers && H % 32 == 0 && E % 4 == 0, "rnn lm: %d layers, hidden_dim %d, embedding_dim %d", L, H, E);
    auto al = [](int64_t n) { return align_up(n, 64); };   // (floats: every part on a 256-byte boundary)
    int64_t total = al((int64_t)V * E);
    for (int k = 0; k < L; k++) total += al((int64_t)4 * H * m.in_dim(k)) + al(4 * H) + al((int64_t)4 * H * H);
    total += al((int64_t)H * Vp) + al(V);
    float* base = static_cast<float*>(dev_alloc((int64_t)sizeof(float) * total));
    try {
        RnnLmDev d;
        d.V = V; d.Vp = Vp; d.E = E; d.H = H; d.L = L; d.sos = m.sos; d.eos = m.eos;
        float* p = base;
        auto put = [&](const float* src, int64_t n) {
            dev_upload(p, src, (int64_t)sizeof(float) * n);
            const float* at = p;
            p += al(n);
            return at;
        };
        d.emb = put(m.emb.data(), (int64_t)V * E);
        std::vector<float> kn;
        for (int k = 0; k < L; k++) {
            d.w_ih[k] = put(m.w_ih[(size_t)k].data(), (int64_t)4 * H * m.in_dim(k));
            d.bias[k] = put(m.bias[(size_t)k].data(), 4 * H);
            kn.resize((size_t)4 * H * H);
            const float* w = m.w_hh[(size_t)k].data();
            for (int g = 0; g < 4 * H; g++)
                for (int i = 0; i < H; i++) kn[(size_t)i * 4 * H + g] = w[(size_t)g * H + i];
            d.whh_kn[k] = put(kn.data(), (int64_t)4 * H * H);
        }
        kn.assign((size_t)H * Vp, 0.f);
        for (int v = 0; v < V; v++)
            for (int i = 0; i < H; i++) kn[(size_t)i * Vp + v] = m.w_out[(size_t)v * H + i];
        d.out_kn = put(kn.data(), (int64_t)H * Vp);
        d.out_b = put(m.b_out.data(), V);
        *out = d;
    } catch (...) {
        try { dev_free(base); } catch (...) {}
        throw;
    }
    return base;
}

// What the fused search needs beyond the rescoring layouts, built when fusion is first switched on for an attached LM: a second
// allocation that the caller owns -- per layer the panels of rnn_lm_fuse_layout.h, the output matrix in torch layout for the GEMM
// launcher, the start state h0 / c0 and row q0 (computed here on the device, once), the debug counters.  *io: the attached LM's tables,
// completed.
void* Engine::rnn_lm_fusion_upload(const RnnLm& m, RnnLmDev* io) {
    K2_HIP(hipSetDevice(device_));
    const int V = m.V, H = m.H, L = m.L;
    K2_REQUIRE(io && io->emb && io->L == L && io->H == H && io->V == V, "rnn lm fusion: the tables are not those of the attached LM");
    auto al = [](int64_t n) { return align_up(n, 64); };
    int64_t total = al((int64_t)V * H) + 2 * al((int64_t)L * H) + al(V) + al(4);
    for (int k = 0; k < L; k++) total += al(rnn_lm_panel_floats(m, k));
    float* base = static_cast<float*>(dev_alloc((int64_t)sizeof(float) * total));
    try {
        RnnLmDev d = *io;
        float* p = base;
        auto room = [&](int64_t n) {
            float* at = p;
            p += al(n);
            return at;
        };
        std::vector<float> kn;
        for (int k = 0; k < L; k++) {
            kn.resize((size_t)rnn_lm_panel_floats(m, k));
            rnn_lm_panels(m, k, kn.data());
            float* at = room((int64_t)kn.size());
            dev_upload(at, kn.data(), (int64_t)sizeof(float) * (int64_t)kn.size());
            d.wcat[k] = at;
        }
        float* wo = room((int64_t)V * H);
        dev_upload(wo, m.w_out.data(), (int64_t)sizeof(float) * V * H);
        d.w_out = wo;
        d.h0 = room((int64_t)L * H);
        d.c0 = room((int64_t)L * H);
        d.q0 = room(V);
        d.work = reinterpret_cast<long long*>(room(4));
        K2_HIP(hipMemsetAsync(d.work, 0, 16, stream_));
        run_sized([&](const Ctx& c) { nlm_start_state(c, d); });
        K2_HIP(hipStreamSynchronize(stream_));
        *io = d;
    } catch (...) {
        try { dev_free(base); } catch (...) {}
        throw;
    }
    return base;
}

void Engine::rnn_lm_fusion_work(int64_t* swept, int64_t* idle) {
    long long w[2] = {0, 0};
    if (rnn_host_ && rnn_dev_.work) {
        K2_HIP(hipSetDevice(device_));
        K2_HIP(hipStreamSynchronize(stream_));
        K2_HIP(copy_blocking(w, rnn_dev_.work, sizeof w, hipMemcpyDeviceToHost));
    }
    if (swept) *swept = w[0];
    if (idle) *idle = w[1];
}

void Engine::nlm_advance_bench(int rows, int H, int iters, float* ms) {
    K2_REQUIRE(rows > 0 && rows <= 4096 && H > 0 && H <= 8192 && H % 32 == 0 && iters > 0 && iters <= 10000 && ms, "nlm_advance_bench: %d rows, hidden_dim %d, %d launches",
               rows, H, iters);
    K2_HIP(hipSetDevice(device_));
    struct Bufs {
        hipStream_t s;
        std::vector<void*> p;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Bufs() {
            (void)hipStreamSynchronize(s);
            for (void* q : p) (void)hipFree(q);
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
        float* take(int64_t n, float scale) {
            float* q = nullptr;
            K2_HIP(hipMalloc(&q, sizeof(float) * (size_t)n));
            p.push_back(q);
            std::vector<float> h((size_t)n);
            uint32_t st = 54321u + (uint32_t)p.size();
            for (auto& v : h) { st = st * 1664525u + 1013904223u; v = (((st >> 8) * (1.0f / 8388608.0f)) - 1.0f) * scale; }
            K2_HIP(copy_blocking(q, h.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice));
            return q;
        }
    } b{stream_, {}};
    // a layer above the first: x = rows of width H, so the launch sums 2 H products per gate (the rescoring step sums H: its input
    // products are one GEMM per time block)
    const float ws = 1.f / sqrtf(2.f * (float)H);
    float *w = b.take(8LL * H * H, ws), *bias = b.take(4LL * H, 1.f), *x = b.take((int64_t)rows * H, 1.f);
    float *h0 = b.take((int64_t)rows * H, 1.f), *h1 = b.take((int64_t)rows * H, 1.f), *c0 = b.take((int64_t)rows * H, 1.f), *c1 = b.take((int64_t)rows * H, 1.f);
    int* idx = reinterpret_cast<int*>(b.take(2LL * rows, 0.f));
    std::vector<int> hi((size_t)2 * rows);
    for (int i = 0; i < rows; i++) { hi[(size_t)i] = (i * 7 + 3) % rows; hi[(size_t)rows + i] = 1; }   // a scattered parent map; every row appends
    K2_HIP(copy_blocking(idx, hi.data(), sizeof(int) * hi.size(), hipMemcpyHostToDevice));
    K2_HIP(hipEventCreate(&b.e0));
    K2_HIP(hipEventCreate(&b.e1));
    Ctx c = make_ctx(false);
    c.instrument = false;
    c.stats = nullptr;
    auto one = [&](int i) {
        NlmAdvance a;
        a.wcat = w; a.bias = bias; a.x_rows = x;
        a.h_par = i & 1 ? h1 : h0; a.c_par = i & 1 ? c1 : c0;
        a.h_out = i & 1 ? h0 : h1; a.c_out = i & 1 ? c0 : c1;
        a.par = idx; a.tok = idx + rows;
        a.M = rows; a.in = H; a.H = H;
        nlm_advance(c, a);
    };
    for (int i = 0; i < 3; i++) one(i);
    K2_HIP(hipEventRecord(b.e0, stream_));
    for (int i = 0; i < iters; i++) one(i);
    K2_HIP(hipEventRecord(b.e1, stream_));
    K2_HIP(hipEventSynchronize(b.e1));
    float t = 0.f;
    K2_HIP(hipEventElapsedTime(&t, b.e0, b.e1));
    *ms = t / iters;
}

void Engine::rnn_lm_score_host(const int64_t* tokens, const int64_t* offsets, int Hn, bool with_eos, float* token_log_probs, float* totals) {
    K2_REQUIRE(rnn_host_, "rnn_lm_score: no LM is attached to the model (k2hip_set_rnn_lm)");
    const RnnLmDev& d = rnn_dev_;
    rnn_lm_check_hyps(d.V, tokens, offsets, Hn, "rnn_lm_score");
    if (Hn == 0) return;
    K2_REQUIRE(totals, "rnn_lm_score: no place for the totals");
    const int64_t cap = tunables().rnn_lm_gx_cap > 0 ? tunables().rnn_lm_gx_cap : kRnnLmGxCapFloats;
    const RnnLmPlan p = rnn_lm_plan(offsets, Hn, with_eos, d.H, cap);
    for (int i = 0; i < Hn; i++) totals[i] = 0.f;
    if (p.R == 0) return;   // (nothing but empty hypotheses without eos: no device work)
    K2_HIP(hipSetDevice(device_));
    const int64_t R = p.R;
    const int H = d.H, E = d.E, L = d.L, G = 4 * H, T = p.T;
    // ONE upload: ids [R] | targets [R] | descriptors [Hn] | base [T + 1]
    const int64_t o_tgt = align_up((int64_t)sizeof(int) * R, 256), o_hyp = o_tgt + align_up((int64_t)sizeof(int) * R, 256),
                  o_base = o_hyp + align_up((int64_t)sizeof(RnnLmHyp) * Hn, 256), nb = o_base + align_up((int64_t)sizeof(long long) * (T + 1), 256);
    char* pin = static_cast<char*>(pinned_in(nb));
    {
        int* ids = reinterpret_cast<int*>(pin);
        int* tgt = reinterpret_cast<int*>(pin + o_tgt);
        RnnLmHyp* hy = reinterpret_cast<RnnLmHyp*>(pin + o_hyp);
        long long* bs = reinterpret_cast<long long*>(pin + o_base);
        for (int t = 0; t <= T; t++) bs[t] = p.base[(size_t)t];
        for (int j = 0; j < Hn; j++) {
            const int orig = p.order[(size_t)j], P = p.npos[(size_t)j];
            const int64_t n = offsets[orig + 1] - offsets[orig];
            const int64_t* y = n ? tokens + offsets[orig] : nullptr;
            hy[j].npos = P; hy[j].orig = orig; hy[j].out_off = p.out_off[(size_t)j];
            for (int t = 0; t < P; t++) {
                const int64_t row = p.base[(size_t)t] + j;
                ids[row] = t == 0 ? d.sos : (int)y[t - 1];
                tgt[row] = t < n ? (int)y[t] : d.eos;
            }
        }
    }
    int max_block_rows = 1;
    for (size_t b = 0; b + 1 < p.block.size(); b++)
        max_block_rows = (int)std::max<int64_t>(max_block_rows, p.base[(size_t)p.block[b + 1]] - p.base[(size_t)p.block[b]]);
    rnn_last_blocks_ = (int)p.block.size() - 1;
    float *d_tlp = nullptr, *d_tot = nullptr;
    // leg timing (set_rnn_lm_timing): events at the legs' borders, read after the call has drained
    std::vector<std::pair<int, hipEvent_t>> marks;   // (leg that ENDS here or -1, event)
    struct Events {
        std::vector<std::pair<int, hipEvent_t>>& m;
        ~Events() {
            for (auto& e : m) (void)hipEventDestroy(e.second);
        }
    } ev_guard{marks};
    auto mark = [&](const Ctx& c, int leg) {
        if (!rnn_timing_ || c.dry) return;
        hipEvent_t e;
        K2_HIP(hipEventCreate(&e));
        marks.emplace_back(leg, e);
        K2_HIP(hipEventRecord(e, c.stream));
    };
    run_sized([&](const Ctx& c) {
        Arena& ar = *c.arena;
        char* blob = ar.take<char>(nb);
        const int* ids = reinterpret_cast<const int*>(blob);
        const int* tgt = reinterpret_cast<const int*>(blob + o_tgt);
        const RnnLmHyp* hy = reinterpret_cast<const RnnLmHyp*>(blob + o_hyp);
        const long long* bs = reinterpret_cast<const long long*>(blob + o_base);
        float* x0 = ar.take<float>(R * E);
        float* y0 = ar.take<float>(R * H);
        float* y1 = L > 1 ? ar.take<float>(R * H) : nullptr;
        float* gx = ar.take<float>((int64_t)max_block_rows * G);
        float* cst = ar.take<float>((int64_t)Hn * H);
        float* lp = ar.take<float>(R);
        d_tlp = ar.take<float>(R);
        d_tot = ar.take<float>(Hn);
        if (!c.dry) K2_HIP(hipMemcpyAsync(blob, pin, (size_t)nb, hipMemcpyHostToDevice, c.stream));
        mark(c, -1);
        rnn_lm_embed(c, d.emb, ids, x0, R, E);
        mark(c, 0);
        const float* in = x0;
        int in_dim = E;
        float* out = y0;
        for (int k = 0; k < L; k++) {
            zero_floats(c, cst, (long long)p.active[0] * H);
            for (size_t b = 0; b + 1 < p.block.size(); b++) {
                const int t0 = p.block[b], t1 = p.block[b + 1];
                const int64_t r0 = p.base[(size_t)t0], rows = p.base[(size_t)t1] - r0;
                mark(c, -1);
                linear(c, in + r0 * in_dim, in_dim, d.w_ih[k], d.bias[k], gx, G, (int)rows, in_dim, G);
                mark(c, 1);
                for (int t = t0; t < t1; t++)
                    rnn_lm_step(c, t ? out + p.base[(size_t)t - 1] * H : nullptr, d.whh_kn[k], gx + (p.base[(size_t)t] - r0) * G, cst,
                                out + p.base[(size_t)t] * H, p.active[(size_t)t], H);
                mark(c, 2);
            }
            c.add_flops(0, 2.0 * (double)R * H * G, 0);
            in = out;
            in_dim = H;
            out = out == y0 ? y1 : y0;
        }
        mark(c, -1);
        rnn_lm_score_rows(c, in, d.out_kn, d.out_b, tgt, lp, R, H, d.V, d.Vp);
        rnn_lm_totals(c, lp, hy, bs, Hn, d_tlp, d_tot);
        mark(c, 3);
    });
    rnn_calls_++;
    const int64_t nb_out = (int64_t)sizeof(float) * (R + Hn);
    float* h_out = static_cast<float*>(pinned(nb_out));
    K2_HIP(hipMemcpyAsync(h_out, d_tlp, sizeof(float) * (size_t)R, hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipMemcpyAsync(h_out + R, d_tot, sizeof(float) * (size_t)Hn, hipMemcpyDeviceToHost, stream_));
    K2_HIP(hipStreamSynchronize(stream_));
    if (token_log_probs) memcpy(token_log_probs, h_out, sizeof(float) * (size_t)R);
    memcpy(totals, h_out + R, sizeof(float) * (size_t)Hn);
    if (rnn_timing_) {
        rnn_ms_ = {0, 0, 0, 0};
        for (size_t i = 1; i < marks.size(); i++) {
            if (marks[i].first < 0) continue;
            float ms = 0.f;
            K2_HIP(hipEventElapsedTime(&ms, marks[i - 1].second, marks[i].second));
            rnn_ms_[(size_t)marks[i].first] += ms;
        }
    }
}

void Engine::rnn_lm_step_bench(int a, int H, int iters, float* fused_ms, float* composed_ms) {
    K2_REQUIRE(a > 0 && a <= 4096 && H > 0 && H <= 8192 && H % 32 == 0 && iters > 0 && iters <= 10000, "rnn_lm_step_bench: %d rows, hidden_dim %d, %d launches",
               a, H, iters);
    K2_HIP(hipSetDevice(device_));
    const int64_t G = 4LL * H;
    struct Bufs {
        hipStream_t s;
        std::vector<void*> p;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Bufs() {
            (void)hipStreamSynchronize(s);
            for (void* q : p) (void)hipFree(q);
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
        float* take(int64_t n, float scale) {
            float* q = nullptr;
            K2_HIP(hipMalloc(&q, sizeof(float) * (size_t)n));
            p.push_back(q);
            std::vector<float> h((size_t)n);
            uint32_t st = 12345u + (uint32_t)p.size();
            for (auto& v : h) { st = st * 1664525u + 1013904223u; v = (((st >> 8) * (1.0f / 8388608.0f)) - 1.0f) * scale; }
            K2_HIP(copy_blocking(q, h.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice));
            return q;
        }
    } b{stream_, {}};
    const float ws = 1.f / sqrtf((float)H);
    float *w = b.take(G * H, ws), *h0 = b.take((int64_t)a * H, 1.f), *h1 = b.take((int64_t)a * H, 1.f), *gx = b.take((int64_t)a * G, 1.f),
          *gh = b.take((int64_t)a * G, 1.f), *cst = b.take((int64_t)a * H, 1.f), *bias = b.take(G, 0.f);
    K2_HIP(hipEventCreate(&b.e0));
    K2_HIP(hipEventCreate(&b.e1));
    Ctx c = make_ctx(false);
    c.instrument = false;
    c.stats = nullptr;
    auto timed = [&](bool fused) {
        auto one = [&](int i) {
            const float *hp = i & 1 ? h1 : h0;
            float* hn = i & 1 ? h0 : h1;
            if (fused) {
                rnn_lm_step(c, hp, w, gx, cst, hn, a, H);
            } else {
                linear(c, hp, H, w, bias, gh, (int)G, a, H, (int)G);
                lstm_cell(c, gx, G, gh, (int)G, cst, hn, a, H);
            }
        };
        for (int i = 0; i < 3; i++) one(i);
        K2_HIP(hipEventRecord(b.e0, stream_));
        for (int i = 0; i < iters; i++) one(i);
        K2_HIP(hipEventRecord(b.e1, stream_));
        K2_HIP(hipEventSynchronize(b.e1));
        float ms = 0.f;
        K2_HIP(hipEventElapsedTime(&ms, b.e0, b.e1));
        return ms / iters;
    };
    if (fused_ms) *fused_ms = timed(true);
    if (composed_ms) *composed_ms = timed(false);
}

}  // namespace k2hip
