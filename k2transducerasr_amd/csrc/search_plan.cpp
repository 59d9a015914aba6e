// The host plans of the four lattice searches: forced alignment (align.hip, ctc_align.hip) and keyword spotting (kws.hip, ctc_kws.hip).
// A plan checks every argument its kernel turns into an address and lays out the call's ONE upload blob (stream descriptors, target ids,
// carried blocks, graph tables).  Host only: the sanitizer builds link this file as it is, and their engine stand-ins (tests/native)
// run the host references on the blob these functions write.
#include <climits>

#include "engine.h"
#include "lattice_ref.h"
#include "ctc_lattice_ref.h"

namespace k2hip {

static_assert(kKwsMaxStates == kKeywordsMaxStates, "the kernel's and the graph builder's state limit are one number");
static_assert(kCtcAlignMaxTokens == kCtcAlignMaxU, "the kernel's and the host reference's target limit are one number");

Engine::AlignPlan Engine::align_plan(int B, int Tp, const int32_t* n_frames, const int64_t* ids, const int32_t* lens, int max_tokens) const {
    const Config& cf = model_->cfg();
    if (cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "align: a CTC model has no transducer lattice");
    K2_REQUIRE(cf.ctx == 2, "align: decoder context size %d (2 is built)", cf.ctx);
    lattice_check_targets(cf.V, B, Tp, n_frames, ids, lens);
    AlignPlan p;
    p.B = B; p.Tp = Tp;
    for (int b = 0; b < B; b++) {
        if (lens[b] > max_tokens) failf(K2HIP_ERR_CAPACITY, "align: stream %d has %d target tokens, max_tokens is %d", b, lens[b], max_tokens);
        K2_REQUIRE(lens[b] <= kAlignMaxU, "align: stream %d has %d target tokens (at most %d)", b, lens[b], kAlignMaxU);
        p.n_ids += lens[b];
        p.n_ctx += lens[b] + 1;
    }
    p.o_ids = align_up((int64_t)sizeof(AlignStream) * B, 16);
    p.o_ctx = align_up(p.o_ids + (int64_t)sizeof(int) * p.n_ids, 16);
    p.blob.assign((size_t)(p.o_ctx + (int64_t)sizeof(long long) * 2 * p.n_ctx), 0);
    AlignStream* st = reinterpret_cast<AlignStream*>(p.blob.data());
    int* h_ids = reinterpret_cast<int*>(p.blob.data() + p.o_ids);
    long long* h_ctx = reinterpret_cast<long long*>(p.blob.data() + p.o_ctx);
    int io = 0, co = 0;
    for (int b = 0; b < B; b++) {
        const int T = n_frames ? n_frames[b] : Tp, U = lens[b];
        st[b] = AlignStream{p.plane_floats, p.bp_words, co, io, U, T};
        p.plane_floats += (long long)T * (U + 1);
        p.bp_words += (long long)T * ((U + 1 + 63) / 64);
        p.max_T = std::max(p.max_T, T);
        p.max_U = std::max(p.max_U, U);
        // the context of position u: the last two ids of [blank, blank, y_1 .. y_u] (the offline beam search's start state)
        long long y0 = K2HIP_BLANK_ID, y1 = K2HIP_BLANK_ID;
        for (int u = 0; u <= U; u++) {
            h_ctx[2 * (co + u)] = y0;
            h_ctx[2 * (co + u) + 1] = y1;
            if (u < U) {
                h_ids[io + u] = (int)ids[io + u];
                y0 = y1;
                y1 = ids[io + u];
            }
        }
        io += U;
        co += U + 1;
    }
    return p;
}

Engine::KwsPlan Engine::kws_plan(int B, int Tp, const KwsIO* io, bool all_frames) const {
    const Config& cf = model_->cfg();
    if (cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "keyword spotting: a CTC model has no transducer lattice");
    K2_REQUIRE(B > 0 && B <= 65535 && Tp >= 1 && io != nullptr, "keyword spotting: bad shape B=%d T'=%d", B, Tp);
    KwsPlan p;
    p.B = B; p.Tp = Tp;
    p.state_off.resize((size_t)B);
    for (int b = 0; b < B; b++) {
        const int T = all_frames ? Tp : io[b].T;
        K2_REQUIRE(io[b].graph && io[b].graph->dec && io[b].a && io[b].start, "keyword spotting: stream %d has no resident graph", b);
        K2_REQUIRE(T >= 0 && T <= Tp, "keyword spotting: stream %d: n_frames %d outside [0, %d]", b, T, Tp);
        K2_REQUIRE(io[b].graph->S >= 1 && io[b].graph->S <= kKwsMaxStates, "keyword spotting: stream %d: %d trie states", b, io[b].graph->S);
        p.state_off[(size_t)b] = p.n_states;
        p.n_states += io[b].graph->S;
    }
    p.o_a = align_up((int64_t)sizeof(KwsStream) * B, 16);
    p.o_st = align_up(p.o_a + (int64_t)sizeof(float) * p.n_states, 16);
    p.blob.assign((size_t)(p.o_st + (int64_t)sizeof(int32_t) * p.n_states), 0);
    KwsStream* st = reinterpret_cast<KwsStream*>(p.blob.data());
    float* h_a = reinterpret_cast<float*>(p.blob.data() + p.o_a);
    int32_t* h_st = reinterpret_cast<int32_t*>(p.blob.data() + p.o_st);
    for (int b = 0; b < B; b++) {
        const int T = all_frames ? Tp : io[b].T, S = io[b].graph->S, so = p.state_off[(size_t)b];
        st[b] = KwsStream{*io[b].graph, p.plane_floats, so, T};
        p.plane_floats += (long long)T * S;
        p.max_T = std::max(p.max_T, T);
        p.max_S = std::max(p.max_S, S);
        memcpy(h_a + so, io[b].a, sizeof(float) * (size_t)S);
        memcpy(h_st + so, io[b].start, sizeof(int32_t) * (size_t)S);
    }
    return p;
}

Engine::CtcKwsPlan Engine::ctc_kws_plan(int B, int Tp, const CtcKwsIO* io, bool all_frames, int V) const {
    const Config& cf = model_->cfg();
    if (!cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "CTC keyword spotting: model_type '%s' has no CTC head", cf.model_type.c_str());
    if (V == 0) V = cf.V;
    K2_REQUIRE(B > 0 && B <= 65535 && Tp >= 1 && V >= 2 && io != nullptr, "CTC keyword spotting: bad shape B=%d T'=%d V=%d", B, Tp, V);
    CtcKwsPlan p;
    p.B = B; p.Tp = Tp; p.V = V;
    p.state_off.resize((size_t)B);
    // the call's distinct graphs (by table block) and where their tables go, in words
    std::vector<const CtcKwsGraph*> graphs;
    std::vector<int> tab_off, graph_of((size_t)B);
    int tab_words = 0;
    for (int b = 0; b < B; b++) {
        const int T = all_frames ? Tp : io[b].T;
        const CtcKwsGraph* g = io[b].graph;
        K2_REQUIRE(g && g->parent && g->tok && g->depth && g->kw && g->bar && g->rc && io[b].v && io[b].st, "CTC keyword spotting: stream %d has no graph", b);
        K2_REQUIRE(T >= 0 && T <= Tp, "CTC keyword spotting: stream %d: n_frames %d outside [0, %d]", b, T, Tp);
        const int S = g->S;
        K2_REQUIRE(S >= 1 && S <= kKwsMaxStates, "CTC keyword spotting: stream %d: %d trie states", b, S);
        size_t k = 0;
        while (k < graphs.size() && graphs[k] != g) k++;
        if (k == graphs.size()) {
            // everything the kernel turns into an address is checked here: parents, tokens, root children
            for (int s = 1; s < S; s++) {
                K2_REQUIRE(g->parent[s] >= 0 && g->parent[s] < s, "CTC keyword spotting: stream %d: parent(%d) = %d", b, s, g->parent[s]);
                K2_REQUIRE(g->tok[s] >= 1 && g->tok[s] < V, "CTC keyword spotting: stream %d: tok(%d) = %d, the log-probs have %d columns", b, s, g->tok[s], V);
                const int r = g->rc[s];
                K2_REQUIRE(r == -1 || (r >= 1 && r < S && g->parent[r] == 0 && g->tok[r] == g->tok[s]), "CTC keyword spotting: stream %d: rc(%d) = %d", b, s, r);
            }
            graphs.push_back(g);
            tab_off.push_back(tab_words);
            tab_words += 6 * S;
        }
        graph_of[(size_t)b] = (int)k;
        const int32_t hold = io[b].st[S], frames = io[b].st[0];
        K2_REQUIRE(hold == -1 || (hold >= 1 && hold < S && g->parent[hold] == 0), "CTC keyword spotting: stream %d carries hold = %d", b, hold);
        K2_REQUIRE(frames >= 0 && (int64_t)frames + T <= INT32_MAX, "CTC keyword spotting: stream %d has run out of frame numbers", b);
        p.state_off[(size_t)b] = p.n_states;
        p.n_states += S;
    }
    p.o_v = align_up((int64_t)sizeof(CtcKwsStream) * B, 16);
    p.o_st = align_up(p.o_v + (int64_t)sizeof(float) * 2 * p.n_states, 16);
    p.o_tab = align_up(p.o_st + (int64_t)sizeof(int32_t) * 2 * p.n_states, 16);
    p.blob.assign((size_t)(p.o_tab + 4 * (int64_t)std::max(tab_words, 1)), 0);
    CtcKwsStream* st = reinterpret_cast<CtcKwsStream*>(p.blob.data());
    float* h_v = reinterpret_cast<float*>(p.blob.data() + p.o_v);
    int32_t* h_st = reinterpret_cast<int32_t*>(p.blob.data() + p.o_st);
    int32_t* h_tab = reinterpret_cast<int32_t*>(p.blob.data() + p.o_tab);
    for (size_t k = 0; k < graphs.size(); k++) {
        const CtcKwsGraph& g = *graphs[k];
        const void* src[6] = {g.parent, g.tok, g.depth, g.kw, g.bar, g.rc};
        for (int j = 0; j < 6; j++) memcpy(h_tab + tab_off[k] + (size_t)j * g.S, src[j], 4 * (size_t)g.S);
    }
    for (int b = 0; b < B; b++) {
        const int T = all_frames ? Tp : io[b].T, S = io[b].graph->S, so = p.state_off[(size_t)b];
        st[b] = CtcKwsStream{tab_off[(size_t)graph_of[(size_t)b]], S, b, so, T};
        p.max_T = std::max(p.max_T, T);
        p.max_S = std::max(p.max_S, S);
        memcpy(h_v + 2 * (size_t)so, io[b].v, sizeof(float) * 2 * (size_t)S);
        memcpy(h_st + 2 * (size_t)so, io[b].st, sizeof(int32_t) * 2 * (size_t)S);
    }
    return p;
}

Engine::CtcAlignPlan Engine::ctc_align_plan(int R, int Tp, const int32_t* n_frames, int H, const int32_t* stream_of, const int64_t* ids,
                                            const int32_t* lens, int max_tokens) const {
    const Config& cf = model_->cfg();
    if (!cf.ctc) failf(K2HIP_ERR_UNSUPPORTED, "ctc_align: model_type '%s' has no CTC head", cf.model_type.c_str());
    ctc_check_targets(cf.V, R, Tp, n_frames, H, stream_of, ids, lens);
    K2_REQUIRE(H <= 65535, "ctc_align: %d targets in one call (at most 65535)", H);
    CtcAlignPlan p;
    p.R = R; p.Tp = Tp; p.H = H;
    for (int h = 0; h < H; h++) {
        if (lens[h] > max_tokens) failf(K2HIP_ERR_CAPACITY, "ctc_align: target %d has %d tokens, max_tokens is %d", h, lens[h], max_tokens);
        K2_REQUIRE(lens[h] <= kCtcAlignMaxU, "ctc_align: target %d has %d tokens (at most %d)", h, lens[h], kCtcAlignMaxU);
        p.n_ids += lens[h];
    }
    p.o_ids = align_up((int64_t)sizeof(CtcAlignTarget) * H, 16);
    p.blob.assign((size_t)(p.o_ids + (int64_t)sizeof(int) * std::max(p.n_ids, 1)), 0);
    CtcAlignTarget* tg = reinterpret_cast<CtcAlignTarget*>(p.blob.data());
    int* h_ids = reinterpret_cast<int*>(p.blob.data() + p.o_ids);
    int io = 0;
    for (int h = 0; h < H; h++) {
        const int r = stream_of ? stream_of[h] : h, T = n_frames ? n_frames[r] : Tp, U = lens[h];
        tg[h] = CtcAlignTarget{p.plane_floats, p.bp_words, r, io, U, T};
        p.plane_floats += (long long)T * (U + 1);
        p.bp_words += (long long)T * ((2 * U + 1 + 63) / 64) * 2;
        p.max_T = std::max(p.max_T, T);
        p.max_U = std::max(p.max_U, U);
        for (int u = 0; u < U; u++) h_ids[io + u] = (int)ids[io + u];
        io += U;
    }
    return p;
}

}  // namespace k2hip
