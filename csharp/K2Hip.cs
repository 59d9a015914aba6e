// P/Invoke declarations for libk2hip.so (include/k2hip.h).
// Source only: there is no dotnet toolchain in the build image, so this file is not compiled here.
using System;
using System.Runtime.InteropServices;

namespace K2TransducerAsr.Hip
{
    [StructLayout(LayoutKind.Sequential)]
    internal struct K2HipModelInfo
    {
        public int vocab_size, context_size, joiner_dim, feature_dim, sample_rate, num_stacks, device, reserved;
    }

    internal static class K2Hip
    {
        private const string Lib = "k2hip";

        [DllImport(Lib)] internal static extern IntPtr k2hip_last_error();
        [DllImport(Lib)] internal static extern int k2hip_model_create(string weightsPath, string overrides, int device, out IntPtr model);
        [DllImport(Lib)] internal static extern int k2hip_model_destroy(IntPtr model);
        [DllImport(Lib)] internal static extern int k2hip_device_count();
        [DllImport(Lib)] internal static extern int k2hip_model_get_info(IntPtr model, out K2HipModelInfo info);
        [DllImport(Lib)] internal static extern long k2hip_fbank_num_frames(IntPtr model, long nSamples);
        [DllImport(Lib)] internal static extern int k2hip_fbank(IntPtr model, float[] samples, long n, float[] feats, long capFrames, out long nFrames);
        [DllImport(Lib)] internal static extern int k2hip_encoder_out_frames(IntPtr model, int T);
        [DllImport(Lib)] internal static extern int k2hip_offline_encoder(IntPtr model, float[] x, long[] xLens, int B, int T,
            float[] encOut, long capFloats, long[] encOutLens, out int Tprime);
        [DllImport(Lib)] internal static extern int k2hip_decoder(IntPtr model, long[] y, int N, float[] decOut);
        [DllImport(Lib)] internal static extern int k2hip_joiner(IntPtr model, float[] enc, float[] dec, int N, float[] logits);
        [DllImport(Lib)] internal static extern int k2hip_offline_greedy(IntPtr model, IntPtr[] feats, long[] nFloats, int B,
            long[] tokens, int[] timestamps, int[] nTokens, int maxTokens);
        [DllImport(Lib)] internal static extern int k2hip_offline_greedy_single(IntPtr model, float[] feats, long nFloats,
            long[] tokens, int[] timestamps, int[] nTokens, int maxTokens);

        // ---- OfflineStream / OfflineRecognizer.GetResults on native streams (include/k2hip.h, "OfflineStream" section): AddSamples queues
        // raw samples, GetResults runs fbank + pad + encoder + search for the whole batch on the device
        [DllImport(Lib)] internal static extern int k2hip_offline_stream_create(IntPtr model, out IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_offline_stream_destroy(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_offline_stream_accept_samples(IntPtr stream, float[] samples, long n);
        [DllImport(Lib)] internal static extern long k2hip_offline_stream_speech_length(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_offline_recognizer_get_results(IntPtr model, IntPtr[] streams, int B);
        [DllImport(Lib)] internal static extern int k2hip_offline_recognizer_get_result(IntPtr model, IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_offline_stream_num_tokens(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_offline_stream_num_timestamps(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_offline_stream_get_tokens(IntPtr stream, long[] tokens, int cap);
        [DllImport(Lib)] internal static extern int k2hip_offline_stream_get_timestamps(IntPtr stream, int[] timestamps, int cap);

        // ---- streaming path (include/k2hip.h, "streaming path" section)
        [DllImport(Lib)] internal static extern int k2hip_online_chunk_info(IntPtr model, out int chunkLength, out int shiftLength, out int framesPerChunk);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_create(IntPtr model, out IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_destroy(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_reset(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_accept_samples(IntPtr stream, float[] samples, long n);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_accept_features(IntPtr stream, float[] feats, long nFrames);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_is_finished(IntPtr stream, int isEndpoint, out int finished);
        [DllImport(Lib)] internal static extern int k2hip_online_step(IntPtr model, IntPtr[] streams, int B, int[] decoded, int[] nNewTokens);
        [DllImport(Lib)] internal static extern int k2hip_online_state_create(IntPtr model, out IntPtr state);
        [DllImport(Lib)] internal static extern int k2hip_online_state_destroy(IntPtr state);
        [DllImport(Lib)] internal static extern long k2hip_online_state_processed_len(IntPtr state);
        [DllImport(Lib)] internal static extern int k2hip_online_encoder(IntPtr model, IntPtr[] states, int B, float[] feats, float[] encoderOut, long capFloats);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_num_tokens(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_num_timestamps(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_get_tokens(IntPtr stream, long[] tokens, int cap);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_get_timestamps(IntPtr stream, int[] timestamps, int cap);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_get_hyp(IntPtr stream, long[] hyp2);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_get_score(IntPtr stream, out float score);
        [DllImport(Lib)] internal static extern int k2hip_beam_stream_create(IntPtr model, int beam, out IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_beam_stream_destroy(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_beam_stream_reset(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_beam_search_chunk(IntPtr model, IntPtr[] streams, int B, float[] encoderOut, int Tc);
        [DllImport(Lib)] internal static extern int k2hip_beam_stream_num_tokens(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_beam_stream_get_tokens(IntPtr stream, long[] tokens, int cap);
        [DllImport(Lib)] internal static extern int k2hip_beam_stream_get_timestamps(IntPtr stream, int[] timestamps, int cap);
        [DllImport(Lib)] internal static extern int k2hip_beam_stream_get_score(IntPtr stream, out float score);
        // N-best hypotheses and token log-probs of the modified beam search (k2hip.h "N-best hypotheses and token log-probs"; INTEGRATION.md)
        [DllImport(Lib)] internal static extern int k2hip_set_nbest(IntPtr model, int n);
        [DllImport(Lib)] internal static extern int k2hip_beam_search_nbest(IntPtr model, float[] encOut, int B, int Tprime, int beam, int nbest, long[] tokens,
                                                                            int[] timestamps, float[] tokenLogProbs, int[] nTokens, int[] nHyps, float[] scores, int maxTokens);
        [DllImport(Lib)] internal static extern int k2hip_offline_stream_num_alternatives(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_offline_stream_get_alternative(IntPtr stream, int i, long[] tokens, int[] timestamps, float[] tokenLogProbs, int cap, out int n, out float score);
        [DllImport(Lib)] internal static extern int k2hip_offline_stream_get_token_log_probs(IntPtr stream, float[] dst, int cap);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_num_alternatives(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_get_alternative(IntPtr stream, int i, long[] tokens, int[] timestamps, float[] tokenLogProbs, int cap, out int n, out float score);
        [DllImport(Lib)] internal static extern int k2hip_online_stream_get_token_log_probs(IntPtr stream, float[] dst, int cap);
        [DllImport(Lib)] internal static extern int k2hip_beam_stream_num_alternatives(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_beam_stream_get_alternative(IntPtr stream, int i, long[] tokens, int[] timestamps, float[] tokenLogProbs, int cap, out int n, out float score);
        [DllImport(Lib)] internal static extern int k2hip_beam_stream_get_token_log_probs(IntPtr stream, float[] dst, int cap);

        [DllImport(Lib)] internal static extern int k2hip_model_meta(IntPtr model, string key, byte[] buf, int cap);
        [DllImport(Lib)] internal static extern int k2hip_set_decoding_method(IntPtr model, string method, int beam);
        // hotword biasing of the offline modified beam search (k2hip.h "hotword biasing"; INTEGRATION.md "Hotwords").  ids: the phrases'
        // token ids back to back, lens: tokens per phrase.  The model copies the tables: destroy the graph after k2hip_set_hotwords.
        [DllImport(Lib)] internal static extern int k2hip_hotwords_create(long[] ids, int[] lens, int nPhrases, float scorePerToken, int vocabSize, out IntPtr hotwords);
        [DllImport(Lib)] internal static extern int k2hip_hotwords_load(IntPtr tokens, string path, float scorePerToken, out IntPtr hotwords);
        [DllImport(Lib)] internal static extern int k2hip_hotwords_destroy(IntPtr hotwords);
        [DllImport(Lib)] internal static extern int k2hip_hotwords_num_states(IntPtr hotwords);
        [DllImport(Lib)] internal static extern int k2hip_hotwords_step(IntPtr hotwords, int state, long token, out int nextState, out float bonus);
        [DllImport(Lib)] internal static extern int k2hip_hotwords_pending(IntPtr hotwords, int state, out float pending);
        [DllImport(Lib)] internal static extern int k2hip_set_hotwords(IntPtr model, IntPtr hotwords /* IntPtr.Zero clears */);
        // n-gram LM shallow fusion in the offline modified beam search (k2hip.h "n-gram LM shallow fusion"; INTEGRATION.md "N-gram LM").
        // ids: the entries' token ids back to back (-1 <s>, -2 </s>, -3 the LM's <unk>), orders: tokens per entry, natural-log weights.
        // The model copies the scaled tables: destroy the LM after k2hip_set_ngram_lm.
        [DllImport(Lib)] internal static extern int k2hip_ngram_lm_create(long[] ids, int[] orders, float[] logProbs, float[] backoffs, long nEntries, int vocabSize, out IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_tokens_load(string tokensPath, out IntPtr tokens);
        [DllImport(Lib)] internal static extern int k2hip_tokens_destroy(IntPtr tokens);
        [DllImport(Lib)] internal static extern int k2hip_ngram_lm_load(IntPtr tokens, string path, out IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_ngram_lm_destroy(IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_ngram_lm_order(IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_ngram_lm_num_states(IntPtr lm);
        [DllImport(Lib)] internal static extern long k2hip_ngram_lm_num_arcs(IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_ngram_lm_start_state(IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_ngram_lm_step(IntPtr lm, int state, long token, out int nextState, out float logProb);
        [DllImport(Lib)] internal static extern int k2hip_set_ngram_lm(IntPtr model, IntPtr lm /* IntPtr.Zero clears */, float scale);
        // Neural LM rescoring (include/k2hip.h "Neural LM rescoring").  The model keeps its own copy: destroy the LM after k2hip_set_rnn_lm.
        [DllImport(Lib)] internal static extern int k2hip_rnn_lm_load(string path, out IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_rnn_lm_destroy(IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_rnn_lm_vocab_size(IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_rnn_lm_embedding_dim(IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_rnn_lm_hidden_dim(IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_rnn_lm_num_layers(IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_rnn_lm_sos_id(IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_rnn_lm_eos_id(IntPtr lm);
        [DllImport(Lib)] internal static extern int k2hip_rnn_lm_score_host(IntPtr lm, long[] tokens, long[] offsets, int hn, int withEos, float[] tokenLogProbs /* may be null */, float[] totals);
        [DllImport(Lib)] internal static extern int k2hip_set_rnn_lm(IntPtr model, IntPtr lm /* IntPtr.Zero clears */, float scale);
        // Neural LM shallow fusion in the streaming modified beam search (include/k2hip.h): the LM's state is carried from chunk to chunk
        [DllImport(Lib)] internal static extern int k2hip_set_rnn_lm_stream_fusion(IntPtr model, int on);
        [DllImport(Lib)] internal static extern int k2hip_rnn_lm_score(IntPtr model, long[] tokens, long[] offsets, int hn, int withEos, float[] tokenLogProbs /* may be null */, float[] totals);
        [DllImport(Lib)] internal static extern int k2hip_offline_stream_get_alternative_lm_score(IntPtr stream, int i, out float lmTotal);
        // streaming: the graph belongs to the stream (IntPtr.Zero detaches; only before the stream's first chunk or after a reset)
        [DllImport(Lib)] internal static extern int k2hip_online_stream_set_hotwords(IntPtr stream, IntPtr hotwords);
        [DllImport(Lib)] internal static extern int k2hip_beam_stream_set_hotwords(IntPtr stream, IntPtr hotwords);

        // voice activity detection and long recordings (include/k2hip.h "Voice activity detection and long recordings"); everything in
        // fbank frames.  Declared here, not compiled in this repository (like the rest of this folder).
        [StructLayout(LayoutKind.Sequential)]
        internal struct VadConfig
        {
            public int band_lo, band_hi, floor_window;
            public float rise, margin, abs_floor;
            public int min_silence, min_speech, speech_pad, max_speech;
        }
        [DllImport(Lib)] internal static extern int k2hip_vad_default_config(IntPtr model, out VadConfig cfg);
        [DllImport(Lib)] internal static extern int k2hip_vad_stream_create(IntPtr model, ref VadConfig cfg, out IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_vad_stream_destroy(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_vad_stream_reset(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_vad_stream_flush(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_vad_accept_features_batch(IntPtr model, IntPtr[] streams, IntPtr[] feats, long[] nFrames, int B);
        [DllImport(Lib)] internal static extern int k2hip_vad_accept_samples_batch(IntPtr model, IntPtr[] streams, int sampleRate, IntPtr[] samples, long[] n, int B);
        [DllImport(Lib)] internal static extern int k2hip_vad_stream_is_speech(IntPtr stream);
        [DllImport(Lib)] internal static extern long k2hip_vad_stream_num_frames(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_vad_stream_num_segments(IntPtr stream);
        [DllImport(Lib)] internal static extern int k2hip_vad_stream_get_segments(IntPtr stream, long[] start, long[] end, int[] forced, int cap);
        [DllImport(Lib)] internal static extern int k2hip_vad_stream_pop_segments(IntPtr stream, int n);
        // cfg: IntPtr.Zero = the defaults (a pinned VadConfig otherwise)
        [DllImport(Lib)] internal static extern int k2hip_offline_recognize_long(IntPtr model, int sampleRate, float[] samples, long n, IntPtr cfg, int maxBatch,
                                                                               long maxBatchFrames, out IntPtr result);
        [DllImport(Lib)] internal static extern int k2hip_long_result_num_segments(IntPtr result);
        [DllImport(Lib)] internal static extern int k2hip_long_result_get_segment(IntPtr result, int i, out long start, out long end, out int forced, out int batch);
        [DllImport(Lib)] internal static extern int k2hip_long_result_get_tokens(IntPtr result, int i, long[] tokens, int[] timestamps, int cap, out int n);
        [DllImport(Lib)] internal static extern int k2hip_long_result_destroy(IntPtr result);

        // Which GPU?  The reference's constructors (OfflineRecognizer.cs:27-28, OnlineRecognizer.cs:18-19) take file paths and nothing
        // else, and they stay as they are: the device rides on the paths.
        //   encoderFilePath "model.k2w@3"                 -> container "model.k2w" on device 3 (the suffix is split off only when what
        //                                                    follows the LAST '@' is 1 - 4 decimal digits: k2hip_parse_model_spec's rule)
        //   decoderFilePath "device=3" (encoder "model.k2w") -> the same; the decoder path is otherwise unused on this route (a .k2w
        //                                                    container holds all three networks)
        // An explicit "@N" wins over "device=N"; neither: device 0.  A host that serves N GPUs builds N recognizers, one per device, from
        // N threads (INTEGRATION.md "More than one GPU"; tests/native/multi_handle_host.c is that host in C).
        internal static void SplitSpec(string encoderFilePath, string decoderFilePath, out string path, out int device)
        {
            path = encoderFilePath;
            device = 0;
            bool fromSpec = false;
            if (!string.IsNullOrEmpty(encoderFilePath))
            {
                int at = encoderFilePath.LastIndexOf('@');
                int nd = encoderFilePath.Length - at - 1;
                if (at > 0 && nd >= 1 && nd <= 4)
                {
                    int d = 0;
                    bool digits = true;
                    for (int i = at + 1; i < encoderFilePath.Length; i++)
                    {
                        char ch = encoderFilePath[i];
                        if (ch < '0' || ch > '9') { digits = false; break; }
                        d = d * 10 + (ch - '0');
                    }
                    if (digits) { path = encoderFilePath.Substring(0, at); device = d; fromSpec = true; }
                }
            }
            if (!fromSpec && !string.IsNullOrEmpty(decoderFilePath) && decoderFilePath.StartsWith("device=", StringComparison.Ordinal))
            {
                if (int.TryParse(decoderFilePath.Substring(7), out int d) && d >= 0) device = d;
            }
        }

        // Is this "encoder file" a .k2w weights container (the engine's format) rather than an ONNX file?  Decided by the file's
        // magic, not by its name, so a renamed container still routes here and an ONNX file never does.  (k2w.py: the file starts
        // with the ASCII bytes "K2W1".)  A "@N" device suffix (SplitSpec) is not part of the file name.
        internal static bool IsK2w(string encoderFilePath)
        {
            SplitSpec(encoderFilePath, null, out string path, out _);
            if (string.IsNullOrEmpty(path) || !System.IO.File.Exists(path)) return false;
            try
            {
                using (var f = System.IO.File.OpenRead(path))
                {
                    var magic = new byte[4];
                    return f.Read(magic, 0, 4) == 4 && magic[0] == (byte)'K' && magic[1] == (byte)'2' && magic[2] == (byte)'W' && magic[3] == (byte)'1';
                }
            }
            catch (System.IO.IOException) { return false; }
        }

        // CustomMetadataMap[key] of the weights container; null when the key is absent (k2hip_model_meta -> K2HIP_ERR_INVALID)
        internal static string Meta(IntPtr model, string key)
        {
            var buf = new byte[4096];
            if (k2hip_model_meta(model, key, buf, buf.Length) != 0) return null;
            int n = Array.IndexOf(buf, (byte)0);
            return System.Text.Encoding.UTF8.GetString(buf, 0, n < 0 ? buf.Length : n);
        }

        internal static void Check(int rc, string what)
        {
            if (rc != 0)
                throw new Exception(what, new Exception(Marshal.PtrToStringAnsi(k2hip_last_error())));
        }
    }
}
