// AddressSanitizer / UBSan driver for the host side of the neural LM shallow fusion: the weight layout of the fused search
// (csrc/rnn_lm_fuse_layout.h) and the switch's bookkeeping in csrc/api.cpp (k2hip_set_rnn_lm_fusion beside k2hip_set_rnn_lm: the second
// allocation made on first use, replaced with the LM, freed with the model) over the CPU stand-ins of the engine (engine_stub*.cpp,
// engine_stub_rnn_lm.cpp, engine_stub_rnn_lm_fusion.cpp).  TEST INFRASTRUCTURE (`make -C k2transducerasr_amd/csrc san_rnn_lm_fusion`,
// tests/test_rnn_lm_fusion_sanitizers.py).
// Exercised: the panels of every layer of every LM file given, into a buffer of exactly the stated size, every element against the
// definition (gate, hidden column and k of each position; zeros in the padding of the input columns, every float written); the switch
// and the LM set, replaced and cleared in every order, with the handle or the model destroyed first.
//   san_rnn_lm_fusion_driver <offline.k2w> <lm.k2w> [<lm.k2w> ...]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/k2hip.h"
#include "../../include/k2hip_debug.h"
#include "../../k2transducerasr_amd/csrc/rnn_lm_fuse_layout.h"

#define CHECK(cond)                                                                                                          \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            fprintf(stderr, "CHECK failed at %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, k2hip_last_error()); \
            exit(3);                                                                                                         \
        }                                                                                                                    \
    } while (0)
#define OK(call) CHECK((call) == K2HIP_OK)

namespace {

void check_layout(const char* path) {
    std::unique_ptr<k2hip::RnnLm> lm(k2hip::rnn_lm_load(path));
    const k2hip::RnnLm& m = *lm;
    for (int k = 0; k < m.L; k++) {
        const int H = m.H, I = m.in_dim(k), Ip = (I + 31) / 32 * 32, Kc = k2hip::rnn_lm_panel_k(m, k);
        CHECK(Kc == Ip + H && k2hip::rnn_lm_panel_floats(m, k) == (int64_t)4 * H * Kc);
        const size_t n = (size_t)k2hip::rnn_lm_panel_floats(m, k);
        std::unique_ptr<float[]> out(new float[n]);   // exactly n floats: a write past the end is a heap overflow
        const float nanv = 0.f / 0.f;
        for (size_t i = 0; i < n; i++) out[i] = nanv;
        k2hip::rnn_lm_panels(m, k, out.get());
        size_t zeros = 0;
        for (size_t i = 0; i < n; i++) {
            CHECK(out[i] == out[i]);                  // every float written
            const size_t jb = i / ((size_t)Kc * 32), r = i % ((size_t)Kc * 32), kq = r / 128, c = (r % 128) / 4, kk = 4 * kq + r % 4;
            const size_t row = (c / 8) * (size_t)H + jb * 8 + c % 8;
            float want = 0.f;
            if (kk < (size_t)I) want = m.w_ih[(size_t)k][row * I + kk];
            else if (kk >= (size_t)Ip) want = m.w_hh[(size_t)k][row * H + (kk - Ip)];
            else zeros++;
            CHECK(memcmp(&out[i], &want, sizeof want) == 0);
        }
        CHECK(zeros == (size_t)4 * H * (Ip - I));
    }
}

void check_switch(const char* model_path, const char* lm_path, const char* lm2_path) {
    for (int order = 0; order < 6; order++) {
        k2hip_model_t* m = nullptr;
        k2hip_rnn_lm_t *lm = nullptr, *lm2 = nullptr;
        int64_t n = -1, sw = -1, idle = -1;
        OK(k2hip_model_create(model_path, nullptr, 0, &m));
        OK(k2hip_rnn_lm_load(lm_path, &lm));
        OK(k2hip_rnn_lm_load(lm2_path, &lm2));
        CHECK(k2hip_set_rnn_lm_fusion(nullptr, 1) != K2HIP_OK);
        OK(k2hip_debug_rnn_lm_fusion_stats(m, &n, &sw, &idle));
        CHECK(n == 0 && sw == 0 && idle == 0);
        OK(k2hip_debug_rnn_lm_fusion_stats(m, nullptr, nullptr, nullptr));
        switch (order) {
            case 0:   // the switch without an LM, then the LM: the layouts come with the LM
                OK(k2hip_set_rnn_lm_fusion(m, 1));
                OK(k2hip_set_rnn_lm(m, lm, 0.5f));
                OK(k2hip_set_rnn_lm(m, lm2, 0.5f));   // replaced while on
                break;
            case 1:   // the LM, then the switch: the layouts on first use, once
                OK(k2hip_set_rnn_lm(m, lm, 0.5f));
                OK(k2hip_set_rnn_lm_fusion(m, 1));
                OK(k2hip_set_rnn_lm_fusion(m, 1));
                OK(k2hip_set_rnn_lm_fusion(m, 0));
                OK(k2hip_set_rnn_lm_fusion(m, 1));
                break;
            case 2:   // cleared while on, set again
                OK(k2hip_set_rnn_lm(m, lm, 0.5f));
                OK(k2hip_set_rnn_lm_fusion(m, 1));
                OK(k2hip_set_rnn_lm(m, nullptr, 0.f));
                OK(k2hip_set_rnn_lm(m, lm2, 0.f));
                break;
            case 3:   // never switched on: nothing but the rescoring layouts
                OK(k2hip_set_rnn_lm(m, lm, 0.5f));
                OK(k2hip_set_rnn_lm_fusion(m, 0));
                break;
            case 4:   // switched off before the LM is replaced
                OK(k2hip_set_rnn_lm(m, lm, 0.5f));
                OK(k2hip_set_rnn_lm_fusion(m, 1));
                OK(k2hip_set_rnn_lm_fusion(m, 0));
                OK(k2hip_set_rnn_lm(m, lm2, 1.f));
                OK(k2hip_set_rnn_lm(m, nullptr, 0.f));
                break;
            default:  // the switch alone
                OK(k2hip_set_rnn_lm_fusion(m, 1));
                OK(k2hip_set_rnn_lm_fusion(m, 0));
                break;
        }
        if (order & 1) {   // the handles first, or the model first
            OK(k2hip_rnn_lm_destroy(lm));
            OK(k2hip_rnn_lm_destroy(lm2));
            OK(k2hip_model_destroy(m));
        } else {
            OK(k2hip_model_destroy(m));
            OK(k2hip_rnn_lm_destroy(lm));
            OK(k2hip_rnn_lm_destroy(lm2));
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s <offline.k2w> <lm.k2w> [<lm.k2w> ...]\n", argv[0]);
        return 2;
    }
    for (int i = 2; i < argc; i++) check_layout(argv[i]);
    check_switch(argv[1], argv[2], argv[argc - 1]);
    printf("san_rnn_lm_fusion_driver ok\n");
    return 0;
}
