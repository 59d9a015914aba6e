// Half-precision operands in the offline Zipformer2 encoder's linear layers (k2hip_set_encoder_precision), host side: which weights
// get f16 panels, and the panels themselves (gemm_f16_layout.h).  No HIP call: the engine uploads the blob, the CPU stand-ins of the
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

void encoder_half_pack(const Model& m, std::vector<uint16_t>* blob, std::vector<EncoderHalfEntry>* entries) {
    const Config& cf = m.cfg();
    if (cf.conformer || cf.zip1 || cf.lstm || cf.streaming)
        failf(K2HIP_ERR_UNSUPPORTED, "set_encoder_precision: only the offline Zipformer2 encoder (zipformer2, zipformer2ctc) has half-precision linear layers");
    if (!blob || !entries) return;   // (the model check alone)
    blob->clear();
    entries->clear();
    for (int si = 0; si < cf.ns; si++)
        for (int li = 0; li < cf.nlayer[si]; li++)
            for (const char* suffix : kHalfSuffixes) {
                char name[160];
                snprintf(name, sizeof name, "encoder.encoders.%d.layers.%d.%s.weight", si, li, suffix);
                if (!m.has(name)) continue;
                const Tensor& t = m.tensor(name);
                if (t.ndim != 2 || t.dims[1] % 32 != 0 || t.dims[1] < 32 || !t.host) continue;   // other K stay on float32
                EncoderHalfEntry e;
                e.name = name;
                e.dev = t.dev;
                e.N = (int)t.dims[0];
                e.K = (int)t.dims[1];
                e.off = (int64_t)blob->size();
                blob->resize(blob->size() + (size_t)gemm_f16_panel_halves(e.N, e.K));
                if (!gemm_f16_pack(t.host, e.N, e.K, blob->data() + e.off))
                    failf(K2HIP_ERR_INVALID, "set_encoder_precision: %s has a weight that is not finite in half precision; the model stays on float32", name);
                entries->push_back(std::move(e));
            }
}

}  // namespace k2hip
