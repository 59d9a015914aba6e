// Loader of the neural LM (rnn_lm_ref.h): a .k2w container with model_type=rnn_lm and the tensors of icefall's RnnLmModel under their
// state-dict names, in torch layout.  Pure host code (no HIP); every extent comes from K2wFile's checked table.
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "k2w_file.h"
#include "rnn_lm_ref.h"

namespace k2hip {

namespace {
int meta_int(const K2wFile& f, const std::string& path, const char* key, long long lo, long long hi) {
    auto it = f.meta.find(key);
    K2_REQUIRE(it != f.meta.end(), "%s: metadata '%s' is missing", path.c_str(), key);
    errno = 0;
    char* end = nullptr;
    const long long v = strtoll(it->second.c_str(), &end, 10);
    K2_REQUIRE(errno == 0 && end != it->second.c_str() && *end == 0, "%s: metadata '%s' = '%s' is not an integer", path.c_str(), key, it->second.c_str());
    K2_REQUIRE(v >= lo && v <= hi, "%s: metadata '%s' = %lld outside [%lld, %lld]", path.c_str(), key, v, lo, hi);
    return (int)v;
}
const K2wTensorRec* find(const K2wFile& f, const std::string& name) {
    for (const K2wTensorRec& r : f.tensors)
        if (r.name == name) return &r;
    return nullptr;
}
// tensor `name` of shape [d0] or [d0][d1] (d1 = 0: one dimension) as float32, every value finite
std::vector<float> take(const K2wFile& f, const std::string& path, const std::string& name, int64_t d0, int64_t d1) {
    const K2wTensorRec* r = find(f, name);
    K2_REQUIRE(r, "%s: tensor '%s' is missing", path.c_str(), name.c_str());
    K2_REQUIRE(r->dtype == 0, "%s: tensor '%s' is not float32", path.c_str(), name.c_str());
    const bool ok = d1 ? (r->ndim == 2 && r->dims[0] == d0 && r->dims[1] == d1) : (r->ndim == 1 && r->dims[0] == d0);
    if (!ok) {
        if (d1) failf(K2HIP_ERR_INVALID, "%s: tensor '%s' has shape [%lld, %lld] (%d dims), expected [%lld, %lld]", path.c_str(), name.c_str(),
                      (long long)r->dims[0], (long long)r->dims[1], r->ndim, (long long)d0, (long long)d1);
        failf(K2HIP_ERR_INVALID, "%s: tensor '%s' has shape [%lld] (%d dims), expected [%lld]", path.c_str(), name.c_str(), (long long)r->dims[0], r->ndim,
              (long long)d0);
    }
    const size_t n = (size_t)(d1 ? d0 * d1 : d0);
    K2_REQUIRE(r->nbytes == n * sizeof(float), "%s: tensor '%s' holds %llu bytes", path.c_str(), name.c_str(), (unsigned long long)r->nbytes);
    std::vector<float> v(n);
    memcpy(v.data(), f.data() + r->off, n * sizeof(float));
    for (size_t i = 0; i < n; i++)
        K2_REQUIRE(std::isfinite(v[i]), "%s: tensor '%s' holds a non-finite value at element %zu", path.c_str(), name.c_str(), i);
    return v;
}
}  // namespace

RnnLm* rnn_lm_load(const std::string& path) {
    K2wFile f(path);
    auto mt = f.meta.find("model_type");
    K2_REQUIRE(mt != f.meta.end() && mt->second == "rnn_lm", "%s: model_type is '%s', not rnn_lm", path.c_str(), mt == f.meta.end() ? "" : mt->second.c_str());
    auto m = std::make_unique<RnnLm>();
    m->V = meta_int(f, path, "vocab_size", 1, 1 << 24);
    m->E = meta_int(f, path, "embedding_dim", 1, 1 << 16);
    m->H = meta_int(f, path, "hidden_dim", 1, 1 << 16);
    m->L = meta_int(f, path, "num_layers", 1, kRnnLmMaxLayers);
    m->tied = meta_int(f, path, "tie_weights", 0, 1) != 0;
    {   // sos_id / eos_id outside [0, V) are refused as such
        const long long big = (long long)1 << 40;
        auto id = [&](const char* key) {
            auto it = f.meta.find(key);
            K2_REQUIRE(it != f.meta.end(), "%s: metadata '%s' is missing", path.c_str(), key);
            errno = 0;
            char* end = nullptr;
            const long long v = strtoll(it->second.c_str(), &end, 10);
            K2_REQUIRE(errno == 0 && end != it->second.c_str() && *end == 0 && v > -big && v < big, "%s: metadata '%s' = '%s' is not an integer", path.c_str(), key,
                       it->second.c_str());
            K2_REQUIRE(v >= 0 && v < m->V, "%s: %s = %lld is outside [0, %d)", path.c_str(), key, v, m->V);
            return (int)v;
        };
        m->sos = id("sos_id");
        m->eos = id("eos_id");
    }
    if (m->H % 32 != 0 || m->E % 4 != 0)
        failf(K2HIP_ERR_UNSUPPORTED, "%s: hidden_dim %d must be a multiple of 32 and embedding_dim %d a multiple of 4", path.c_str(), m->H, m->E);
    const int V = m->V, E = m->E, H = m->H;
    m->emb = take(f, path, "input_embedding.weight", V, E);
    for (int k = 0; k < m->L; k++) {
        const std::string s = std::to_string(k);
        m->w_ih.push_back(take(f, path, "rnn.weight_ih_l" + s, 4 * H, m->in_dim(k)));
        m->w_hh.push_back(take(f, path, "rnn.weight_hh_l" + s, 4 * H, H));
        std::vector<float> bi = take(f, path, "rnn.bias_ih_l" + s, 4 * H, 0), bh = take(f, path, "rnn.bias_hh_l" + s, 4 * H, 0);
        for (size_t i = 0; i < bi.size(); i++) bi[i] = bi[i] + bh[i];
        m->bias.push_back(std::move(bi));
    }
    if (m->tied && !find(f, "output_linear.weight")) {
        K2_REQUIRE(E == H, "%s: tie_weights needs embedding_dim == hidden_dim (%d, %d) when 'output_linear.weight' is absent", path.c_str(), E, H);
        m->w_out = m->emb;
    } else {
        m->w_out = take(f, path, "output_linear.weight", V, H);
    }
    m->b_out = take(f, path, "output_linear.bias", V, 0);
    return m.release();
}

}  // namespace k2hip
