// The other halves of `partial class OnlineRecognizer` and `partial class OnlineStream`: what routes the STREAMING hot path
// to libk2hip.so.  Source only (no dotnet toolchain in the build image).
//
// How it plugs into the reference tree (csharp/patches/OnlineRecognizer.cs.patch and OnlineStream.cs.patch are the exact
// edits; `patch -p1` applies them):
//   * OnlineRecognizer.cs:11  `public class OnlineRecognizer` -> `public partial class OnlineRecognizer`
//   * OnlineRecognizer.cs:21  IN FRONT of `OnlineModel onlineModel = new OnlineModel(encoderFilePath, ...)`:
//         if (Hip.K2Hip.IsK2w(encoderFilePath)) { InitHip(encoderFilePath, decoderFilePath, tokensFilePath, decodingMethod, sampleRate, featureDim); return; }
//     (`new OnlineModel` opens ONNXRuntime sessions on the path, OnlineModel.cs:28-30,224-228, and leaves `CustomMetadata` null
//     without an encoder session, :32 -- the switch at :26 would dereference it.)  `onlineModel` is a local of the constructor
//     (:21-44): nothing behind the constructor uses it, so there is no other use site to serve.
//   * OnlineRecognizer.cs:62  CreateOnlineStream: `if (_hipModel != null && _hipFused) return new OnlineStream(_hipModel);`
//   * OnlineRecognizer.cs:499 Dispose: `_hipModel?.Dispose();` BEHIND the closing brace of `if (_onlineProj != null) { _onlineProj.Dispose(); }` --
//     after the operator (OnlineProjOfHip borrows the handle) but not inside that block: on the fused route `_onlineProj` is null and the
//     block is skipped, and the model (weights, arenas, the streams' state pool) must be released all the same
//   * WHICH GPU: the constructor keeps its signature; the device rides on the paths (K2Hip.SplitSpec): encoderFilePath "model.k2w@3", or
//     decoderFilePath "device=3" -- unused otherwise on this route.  Streams are pinned to the recognizer's GPU at CreateOnlineStream time
//     (OnlineRecognizer.cs:60-64); a host spreads its streams over N recognizers, stream id mod N (SURVEY 8e, INTEGRATION.md)
//   * OnlineStream.cs:7       `public class OnlineStream` -> `public partial class OnlineStream`
//   * OnlineStream.cs:59,126  AddSamples / IsFinished forward to the native stream when it exists; :164 Dispose destroys it
//
// The reference's IOnlineProj contract (IOnlineProj.cs:65-71) moves every stream's caches through managed arrays each tick
// (GetEncoderInitStates / stack_states / EncoderProj / unstack_states).  On the GPU the caches never leave HBM, so the unit of the
// fast route is the STREAM: an OnlineStream that owns a native handle, and one delegate that replaces ForwardBatchGreedySearch
// (OnlineRecognizer.cs:85-219) by one k2hip_online_step per tick.
//
// decodingMethod on a .k2w model:
//   "greedy_search" (default)    the fused route above (any streaming model type of the container, CTC included: k2hip_online_step
//                                runs the model's own search, as :33-36 would select it)
//   "greedy_search_operators"    the reference's UNCHANGED loop (:85-219) over OnlineProjOfHip's operators (csharp/OnlineProjOfHip.cs;
//                                streaming Zipformer2 transducers only), for A/B comparisons against the ONNX path
//   "modified_beam_search"       the fused route under k2hip_set_decoding_method(.., beam 4): hypotheses carried from chunk to chunk
//                                (no reference counterpart; include/k2hip.h).  Tokens / Timestamps are re-read after every step (the
//                                best hypothesis can revise earlier tokens); timestamps are absolute frame indexes
using System;
using System.Collections.Generic;
using System.IO;
using System.Linq;
using K2TransducerAsr.Hip;

namespace K2TransducerAsr
{
    internal sealed class HipOnlineModel : IDisposable
    {
        internal IntPtr Handle;
        internal int ChunkLength, ShiftLength, FramesPerChunk;

        internal HipOnlineModel(string k2wPath, int device = 0)
        {
            // (OnlineModel.cs:101-106's `comment` -> "...ctc" rule and the decoder / joiner metadata are applied by the library when it
            // reads the container: csrc/model.cpp)
            K2Hip.Check(K2Hip.k2hip_model_create(k2wPath, null, device, out Handle), "OnlineRecognizer: model load failed");
            K2Hip.Check(K2Hip.k2hip_online_chunk_info(Handle, out ChunkLength, out ShiftLength, out FramesPerChunk),
                        "OnlineRecognizer: not a streaming model");
        }
        public void Dispose() { if (Handle != IntPtr.Zero) { K2Hip.k2hip_model_destroy(Handle); Handle = IntPtr.Zero; } }
    }

    // the members OnlineStream gains (partial class): the native stream replaces _states, _wavFrontend and the
    // feature FIFO; Hyp / Tokens / Timestamps keep their managed types and are refreshed after every step.
    public partial class OnlineStream
    {
        internal IntPtr HipStream = IntPtr.Zero;

        internal OnlineStream(HipOnlineModel model)
        {
            K2Hip.Check(K2Hip.k2hip_online_stream_create(model.Handle, out HipStream), "OnlineStream: create failed");
            _hyp = new Int64[] { 0, 0 };                     // OnlineStream.cs:43-45
            _tokens = new List<Int64> { 0, 0 };
        }

        // AddSamples (:57-79), IsFinished (:124-161) forward when HipStream != IntPtr.Zero:
        internal void AddSamplesHip(float[] samples) =>
            K2Hip.Check(K2Hip.k2hip_online_stream_accept_samples(HipStream, samples, samples.LongLength), "AddSamples failed");

        // Samples at any rate (include/k2hip.h "Input at other sample rates"): the native stream carries the resampler's state, so any
        // chunking gives the same frames.  The rate is fixed by the stream's first samples until it is reset; native streams only.
        [System.Runtime.InteropServices.DllImport("k2hip")]
        private static extern int k2hip_online_stream_accept_waveform(IntPtr stream, int sampleRate, float[] samples, long n);
        public void AddSamples(float[] samples, int sampleRate)
        {
            if (HipStream == IntPtr.Zero) throw new NotSupportedException("AddSamples(samples, sampleRate) needs the HIP backend");
            K2Hip.Check(k2hip_online_stream_accept_waveform(HipStream, sampleRate, samples, samples.LongLength), "AddSamples failed");
        }

        internal bool IsFinishedHip(bool isEndpoint)
        {
            K2Hip.Check(K2Hip.k2hip_online_stream_is_finished(HipStream, isEndpoint ? 1 : 0, out int fin), "IsFinished failed");
            return fin != 0;
        }

        // This stream's hotword list under modified_beam_search (k2hip.h "hotword biasing", STREAMING): token-id phrases, back to
        // back in `ids` with `lens` tokens each; null detaches.  Only before the stream's first decoded chunk.  The native stream
        // keeps its own reference to the uploaded tables, so the graph is destroyed here at once.
        public void SetHotwords(long[] ids, int[] lens, float scorePerToken, int vocabSize)
        {
            if (HipStream == IntPtr.Zero) throw new InvalidOperationException("SetHotwords: not a libk2hip stream");
            if (ids == null || lens == null)
            {
                K2Hip.Check(K2Hip.k2hip_online_stream_set_hotwords(HipStream, IntPtr.Zero), "SetHotwords failed");
                return;
            }
            K2Hip.Check(K2Hip.k2hip_hotwords_create(ids, lens, lens.Length, scorePerToken, vocabSize, out IntPtr graph), "SetHotwords: bad phrase list");
            try { K2Hip.Check(K2Hip.k2hip_online_stream_set_hotwords(HipStream, graph), "SetHotwords failed"); }
            finally { K2Hip.k2hip_hotwords_destroy(graph); }
        }

        // Dispose(bool) (:162-190) calls this first
        internal void DisposeHip()
        {
            if (HipStream != IntPtr.Zero) { K2Hip.k2hip_online_stream_destroy(HipStream); HipStream = IntPtr.Zero; }
        }

        internal void PullResultsHip()
        {
            int n = K2Hip.k2hip_online_stream_num_tokens(HipStream);
            var tok = new long[n];
            K2Hip.Check(K2Hip.k2hip_online_stream_get_tokens(HipStream, tok, n), "get_tokens failed");
            int m = K2Hip.k2hip_online_stream_num_timestamps(HipStream);
            var ts = new int[m];
            K2Hip.Check(K2Hip.k2hip_online_stream_get_timestamps(HipStream, ts, m), "get_timestamps failed");
            _tokens = tok.ToList();                          // OnlineRecognizer.cs:209
            _timestamps = ts.ToList();                       // :210 (the native list already holds the AddRange result)
            K2Hip.Check(K2Hip.k2hip_online_stream_get_hyp(HipStream, _hyp), "get_hyp failed");   // :208
        }

        // N-best and token confidences (k2hip.h "N-best hypotheses and token log-probs"; on after the recognizer's SetNbest(n > 1)):
        // the stream's alternatives in pick order -- entry 0 is the result Tokens / Timestamps report -- each with its tokens (no blank
        // prefix), frame indexes, token log-probs (unbiased by hotwords, <= 0) and finalized log-prob.
        public sealed class Alternative
        {
            public long[] Tokens;
            public int[] Timestamps;
            public float[] TokenLogProbs;
            public float Score;
        }
        public int NumAlternatives
        {
            get
            {
                if (HipStream == IntPtr.Zero) throw new InvalidOperationException("NumAlternatives: not a libk2hip stream");
                int n = K2Hip.k2hip_online_stream_num_alternatives(HipStream);
                if (n < 0) K2Hip.Check(n, "num_alternatives failed");
                return n;
            }
        }
        public Alternative GetAlternative(int i)
        {
            if (HipStream == IntPtr.Zero) throw new InvalidOperationException("GetAlternative: not a libk2hip stream");
            // the length first (no buffer is written with cap = 0 unless the alternative is empty), then the copy
            int rc = K2Hip.k2hip_online_stream_get_alternative(HipStream, i, null, null, null, int.MaxValue, out int n, out float score);
            K2Hip.Check(rc, "get_alternative failed");
            var a = new Alternative { Tokens = new long[n], Timestamps = new int[n], TokenLogProbs = new float[n], Score = score };
            if (n > 0)
                K2Hip.Check(K2Hip.k2hip_online_stream_get_alternative(HipStream, i, a.Tokens, a.Timestamps, a.TokenLogProbs, n, out n, out score), "get_alternative failed");
            return a;
        }
        public List<Alternative> Alternatives
        {
            get
            {
                var list = new List<Alternative>();
                for (int i = 0, n = NumAlternatives; i < n; i++) list.Add(GetAlternative(i));
                return list;
            }
        }
        // token log-probs of the best result, parallel to its emitted tokens
        public float[] TokenLogProbs => GetAlternative(0).TokenLogProbs;
    }

    public partial class OnlineRecognizer
    {
        private HipOnlineModel _hipModel;
        private bool _hipFused;

        // N-best: n > 1 makes every step under "modified_beam_search" keep up to n alternatives, each with its token log-probs, on
        // every stream (OnlineStream.Alternatives / TokenLogProbs; re-read them after every step, as Tokens); 1 = off.
        public void SetNbest(int n)
        {
            if (_hipModel == null) throw new InvalidOperationException("SetNbest: not a libk2hip recognizer");
            K2Hip.Check(K2Hip.k2hip_set_nbest(_hipModel.Handle, n), "SetNbest failed");
        }
        public List<OnlineStream.Alternative> GetAlternatives(OnlineStream stream) { return stream.Alternatives; }

        // sherpa's lm / lm_scale for an n-gram: a text ARPA file over the token strings of tokens.txt, fused into modified_beam_search
        // (k2hip.h "n-gram LM shallow fusion"); arpaPath = null clears.  A stream keeps the LM it decoded its first chunk with: set it
        // before the streams start, or reset them afterwards.
        public void SetNgramLm(string arpaPath, float scale)
        {
            if (_hipModel == null) throw new InvalidOperationException("SetNgramLm: not a libk2hip recognizer");
            if (arpaPath == null)
            {
                K2Hip.Check(K2Hip.k2hip_set_ngram_lm(_hipModel.Handle, IntPtr.Zero, 0f), "SetNgramLm failed");
                return;
            }
            K2Hip.Check(K2Hip.k2hip_tokens_load(_tokensFilePath, out IntPtr tokens), "SetNgramLm: tokens");
            try
            {
                K2Hip.Check(K2Hip.k2hip_ngram_lm_load(tokens, arpaPath, out IntPtr lm), "SetNgramLm: load failed");
                try { K2Hip.Check(K2Hip.k2hip_set_ngram_lm(_hipModel.Handle, lm, scale), "SetNgramLm failed"); }
                finally { K2Hip.k2hip_ngram_lm_destroy(lm); }
            }
            finally { K2Hip.k2hip_tokens_destroy(tokens); }
        }
        private string _tokensFilePath;   // (SetNgramLm reads the ARPA words through the same token table)

        // the constructor's early branch (see the header): everything :21-57 does, for a .k2w container
        private void InitHip(string encoderFilePath, string decoderFilePath, string tokensFilePath, string decodingMethod, int sampleRate, int featureDim)
        {
            K2Hip.SplitSpec(encoderFilePath, decoderFilePath, out string k2wPath, out int device);
            _hipModel = new HipOnlineModel(k2wPath, device);
            _tokens = File.ReadAllLines(tokensFilePath);                                // :24
            _tokensFilePath = tokensFilePath;
            _hipFused = decodingMethod != "greedy_search_operators";
            if (decodingMethod == "modified_beam_search")
                K2Hip.Check(K2Hip.k2hip_set_decoding_method(_hipModel.Handle, "modified_beam_search", 4), "OnlineRecognizer: decoding method");
            if (_hipFused)
            {
                _forwardBatch = new ForwardBatchOnline(this.ForwardBatchGreedySearchHip);
                // _onlineProj stays null: the loops that dereference it (:91-204, :226-305) are not bound, CreateOnlineStream returns
                // the native-handle stream, Dispose (:496) checks for null -- and releases _hipModel behind that check, not inside it
            }
            else
            {
                var proj = new OnlineProjOfHip(_hipModel);                              // borrows the handle; :26-44's selection
                proj.SampleRate = sampleRate;                                           // :23
                _onlineProj = proj;
                _forwardBatch = new ForwardBatchOnline(this.ForwardBatchGreedySearch);  // the reference's own loop, :48-50
            }
        }

        // replaces ForwardBatchGreedySearch (:85-219): GetDecodeChunk, stack_states, EncoderProj, the 8-frame
        // greedy loop, unstack_states and RemoveChunk are one native call; streams without a full chunk are
        // removed from the caller's list exactly as :117-120 does.
        private void ForwardBatchGreedySearchHip(List<OnlineStream> streams)
        {
            if (streams.Count == 0) return;
            try
            {
                int B = streams.Count;
                var handles = streams.Select(s => s.HipStream).ToArray();
                var decoded = new int[B];
                var nNew = new int[B];
                K2Hip.Check(K2Hip.k2hip_online_step(_hipModel.Handle, handles, B, decoded, nNew), "Online recognition failed");
                var skipped = new List<OnlineStream>();
                for (int i = 0; i < B; i++)
                {
                    if (decoded[i] == 0) skipped.Add(streams[i]);
                    else streams[i].PullResultsHip();
                }
                foreach (var s in skipped) streams.Remove(s);
            }
            catch (Exception ex)
            {
                throw new Exception("Online recognition failed", ex);       // same outer message as :214-217
            }
        }
    }
}
