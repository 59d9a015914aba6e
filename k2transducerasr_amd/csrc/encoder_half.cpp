// Half-precision operands in the offline Zipformer2 encoder's linear layers (k2hip_set_encoder_precision) and in the offline Conformer's
// (k2hip_set_conformer_precision), host side: which weights get f16 panels, and the panels themselves (gemm_f16_layout.h).  No HIP call: the engine uploads the blob, the CPU stand-ins of the
// sanitizer builds run the same routine.
#include "engine.h"
#include "gemm_f16_layout.h"

namespace k2hip {

// The 2-D encoder.* weights the offline layer body (Engine::encoder_layer) hands to linear() under their plain names.  Not here:
// feed_forward1.in_proj (stacked with the attention weights' in_proj, "#ff1_attn_in"), feed_forward2.out_proj (its launch carries the
// bypass mix), the "#glu" repacks, encoder_embed, the positional projections, and everything outside the encoder.
static const char* const kHalfSuffixes[] = {
    "feed_forward1.out_proj", "feed_forward2.in_proj", "feed_forward3.in_proj", "feed_forward3.out_proj",
    "nonlin_attention.in_proj", "nonlin_attention.out_proj", "self_attn1.in_proj", "self_attn1.out_proj",
    "self_attn2.in_proj", "self_attn2.out_proj", "conv_module1.in_proj", "conv_module1.out_proj",
    "conv_module2.in_proj", "conv_module2.out_proj",
};

// Level 2 adds the weights of the layer body's other launches, under the names the engine asks the model for: the stacked
// [feed_forward1.in_proj ; self_attn_weights.in_proj] and the row-interleaved "#glu" in_proj copies (model.cpp add_repacks keeps their
// host copies, so the panels hold exactly the rows the float32 launches read), and feed_forward2.out_proj.
static const char* const kHalfNames2[] = {
    "#ff1_attn_in.weight", "nonlin_attention.in_proj.weight#glu", "conv_module1.in_proj.weight#glu", "conv_module2.in_proj.weight#glu",
    "feed_forward2.out_proj.weight",
};

// Level 3 adds encoder_embed's matrix work (Engine::encoder_embed): the third convolution as the engine's implicit GEMM reads it
// ("#ohwi": [Co][kt][kf][ci]), the ConvNeXt pointwise pair (1 x 1 convolutions: [N, K, 1, 1] is the [N, K] matrix) and the output Linear
// in NHWC flatten order ("#fc").  conv.4 (K = 72) and conv.0 have no f16 form.
static const char* const kHalfEmbed3[] = {
    "encoder_embed.conv.7.weight#ohwi", "encoder_embed.convnext.pointwise_conv1.weight", "encoder_embed.convnext.pointwise_conv2.weight",
    "encoder_embed.out.weight#fc",
};

// The checkpoint tensor behind row `row` of a repacked weight, for the refusal's message.
static std::string source_name(const Model& m, const std::string& prefix, const std::string& suffix, int row) {
    if (suffix == "#ff1_attn_in.weight") {
        const int F1 = (int)m.tensor(prefix + "feed_forward1.in_proj.weight").dims[0];
        return prefix + (row < F1 ? "feed_forward1.in_proj.weight" : "self_attn_weights.in_proj.weight");
    }
    const size_t cut = suffix.find("#glu");
    return prefix + (cut == std::string::npos ? suffix : suffix.substr(0, cut));
}

// One weight into the blob: N = its rows, K = everything behind them.  Not a matrix, K % 32 != 0 or no host copy: it stays on float32 and
// nothing is added.  `source(row)` names the checkpoint tensor of a row for the refusal, `who` the switch.
template <class Source>
static void add_panels(const Model& m, const std::string& name, Source&& source, const char* who, std::vector<uint16_t>* blob,
                       std::vector<EncoderHalfEntry>* entries) {
    if (!m.has(name)) return;
    const Tensor& t = m.tensor(name);
    int64_t K = 1;
    for (int d = 1; d < t.ndim; d++) K *= t.dims[d];
    // [N, K], or a 1 x 1 convolution ([N, K, 1, 1]) or a pointwise Conv1d ([N, K, 1]): the [N, K] matrix
    const bool matrix = t.ndim == 2 || (t.ndim == 4 && t.dims[2] == 1 && t.dims[3] == 1) || (t.ndim == 3 && t.dims[2] == 1);
    if (!matrix || K % 32 != 0 || K < 32 || !t.host) return;   // other K stay on float32
    EncoderHalfEntry e;
    e.name = name;
    e.dev = t.dev;
    e.N = (int)t.dims[0];
    e.K = (int)K;
    e.off = (int64_t)blob->size();
    blob->resize(blob->size() + (size_t)gemm_f16_panel_halves(e.N, e.K));
    if (!gemm_f16_pack(t.host, e.N, e.K, blob->data() + e.off)) {
        int row = 0;   // the first row with such a weight: which checkpoint tensor a repacked row came from
        std::vector<uint16_t> one((size_t)gemm_f16_panel_halves(1, e.K));
        while (row < e.N - 1 && gemm_f16_pack(t.host + (size_t)row * e.K, 1, e.K, one.data())) row++;
        failf(K2HIP_ERR_INVALID, "%s: %s has a weight that is not finite in half precision; the model stays as it was", who, source(row).c_str());
    }
    entries->push_back(std::move(e));
}

void encoder_half_pack(const Model& m, std::vector<uint16_t>* blob, std::vector<EncoderHalfEntry>* entries, int level) {
    const Config& cf = m.cfg();
    if (cf.conformer || cf.zip1 || cf.lstm || cf.streaming)
        failf(K2HIP_ERR_UNSUPPORTED, "set_encoder_precision: only the offline Zipformer2 encoder (zipformer2, zipformer2ctc) has half-precision linear layers");
    if (!blob || !entries) return;   // (the model check alone)
    blob->clear();
    entries->clear();
    std::vector<std::string> suffixes;
    for (const char* suffix : kHalfSuffixes) suffixes.push_back(std::string(suffix) + ".weight");
    if (level >= 2) suffixes.insert(suffixes.end(), std::begin(kHalfNames2), std::end(kHalfNames2));
    const char* who = "set_encoder_precision";
    for (int si = 0; si < cf.ns; si++)
        for (int li = 0; li < cf.nlayer[si]; li++)
            for (const std::string& suffix : suffixes) {
                char prefix[96];
                snprintf(prefix, sizeof prefix, "encoder.encoders.%d.layers.%d.", si, li);
                add_panels(m, prefix + suffix, [&](int row) { return source_name(m, prefix, suffix, row); }, who, blob, entries);
            }
    if (level >= 3)
        for (const std::string name : kHalfEmbed3) add_panels(m, name, [&](int) { return name.substr(0, name.find('#')); }, who, blob, entries);
}

// The offline Conformer (k2hip_set_conformer_precision): the eight weights Engine::conformer_layer hands to linear() -- the two
// feed-forward pairs, the attention's in_proj and out_proj, the conv module's pointwise pair ([N, K, 1]).  All under their checkpoint
// names.  Not here: linear_pos (its product is cached per length), Conv2dSubsampling with its output Linear, the encoder's output
// projection.  The levels 1 and 2 have the same panels: level 2 adds kernels (conformer_f16.hip), no weight.
static const char* const kConformerSuffixes[] = {
    "feed_forward_macaron.0", "feed_forward_macaron.4", "feed_forward.0", "feed_forward.4",
    "self_attn.in_proj", "self_attn.out_proj", "conv_module.pointwise_conv1", "conv_module.pointwise_conv2",
};

void conformer_half_pack(const Model& m, std::vector<uint16_t>* blob, std::vector<EncoderHalfEntry>* entries) {
    const Config& cf = m.cfg();
    if (!cf.conformer || cf.streaming)
        failf(K2HIP_ERR_UNSUPPORTED, "set_conformer_precision: only the offline Conformer encoder (conformer) has this switch");
    if (!blob || !entries) return;   // (the model check alone)
    blob->clear();
    entries->clear();
    for (int li = 0; li < cf.nlayer[0]; li++)
        for (const char* suffix : kConformerSuffixes) {
            char prefix[96];
            snprintf(prefix, sizeof prefix, "encoder.encoder.layers.%d.", li);
            const std::string name = std::string(prefix) + suffix + ".weight";
            add_panels(m, name, [&](int) { return name; }, "set_conformer_precision", blob, entries);
        }
}

}  // namespace k2hip
