// The other halves of `partial class OfflineRecognizer` and `partial class OfflineStream`: what routes OfflineRecognizer's hot path
// to libk2hip.so.  Source only (no dotnet toolchain in the build image).
//
// How it plugs into the reference tree (csharp/patches/OfflineRecognizer.cs.patch and OfflineStream.cs.patch are the exact edits;
// `patch -p1` applies them):
//   * OfflineRecognizer.cs:12   `public class OfflineRecognizer`  ->  `public partial class OfflineRecognizer`
//   * OfflineRecognizer.cs:30   IN FRONT of `_offlineModel = new OfflineModel(encoderFilePath, ...)`:
//         if (Hip.K2Hip.IsK2w(encoderFilePath)) { InitHip(encoderFilePath, decoderFilePath, tokensFilePath, decodingMethod, sampleRate, featureDim); return; }
//     The branch cannot live in the Proj switch at :38-53: `new OfflineModel` (:30) has by then handed the path to
//     `new InferenceSession(path)` (OfflineModel.cs:25,111-115), which throws on a .k2w, and the switch key
//     `_offlineModel.CustomMetadata.Model_type` only exists once ONNX metadata was read.
//   * OfflineRecognizer.cs:73   CreateOfflineStream: `if (_hipSamples) return new OfflineStream((OfflineProjOfHip)_offlineProj, _offlineModel.CustomMetadata);`
//   * OfflineStream.cs:7        `public class OfflineStream` -> `public partial class OfflineStream`
//   * OfflineStream.cs:45       AddSamples, IN FRONT of `lock (obj)`: `if (HipStream != IntPtr.Zero) { AddSamplesHip(samples); return; }`
//   * OfflineStream.cs:73       Dispose(bool): `DisposeHip();`
// Nothing else changes.  Every later use of `_offlineModel` in OfflineRecognizer.cs reads `CustomMetadata` only:
//   :31  FeatureDim (set again by InitHip)      :73  CreateOfflineStream -> new OfflineStream(_offlineModel.CustomMetadata, ...)
//   :95, :191, :307, :367  `_offlineModel.CustomMetadata.Context_size` at the top of the four Forward* loops
// InitHip serves them by constructing `new OfflineModel("", "", "", n)` -- initModel returns null for an empty path
// (OfflineModel.cs:86-89), so no session is opened and the `!= null` guards at :31-72 skip the metadata reads -- and assigning the
// engine's metadata (filled from k2hip_model_get_info / k2hip_model_meta) to its settable `CustomMetadata` (:78).
// Dispose (:586-611) already calls `_offlineProj.Dispose()`, which is OfflineProjOfHip.Dispose -> k2hip_model_destroy.
//
// WHERE THE FBANK RUNS.  The reference computes it on the CPU inside OfflineStream.AddSamples (`_wavFrontend.GetFbank(samples)`,
// OfflineStream.cs:47) under a process-wide static lock (:16,45): 32 utterances of a batch are 32 serialized CPU fbanks before GetResults
// starts.  On the fused route a stream owns a NATIVE stream (k2hip_offline_stream_*): AddSamples hands the raw samples over (a copy, no
// lock, no `_wavFrontend`), `OfflineInputEntity.SpeechLength` is kept equal to what the reference would show (80 x the frame count of
// the samples so far: k2hip_offline_stream_speech_length), and GetResults is ONE native call for the batch --
// k2hip_offline_recognizer_get_results: samples H2D, one batched fbank launch, pad, encoder, search, tokens D2H -- after which the
// native stream holds Tokens / Timestamps exactly as OfflineRecognizer.cs:250-296 leaves them (2 x B blank prefix, Timestamps.AddRange,
// RemoveSamples) and this file copies them into the managed lists.
//
// WHICH GPU.  The constructors keep their signatures; the device rides on the paths (K2Hip.SplitSpec): encoderFilePath
// "model.k2w@3", or decoderFilePath "device=3" -- unused otherwise on this route.  INTEGRATION.md "More than one GPU".
//
// decodingMethod on a .k2w model:
//   "greedy_search" (default)    the fused delegates below: fbank + pad + encoder + loop are ONE native call per batch
//   "modified_beam_search"       the same entry under k2hip_set_decoding_method(.., beam 4) (BASELINE configs[2]; no reference counterpart)
//   "greedy_search_operators"    the reference's UNCHANGED loops (:93-303) over OfflineProjOfHip's three operators (one native call
//                                per frame) with the reference's own managed streams (CPU fbank) -- for A/B comparisons against the ONNX path
//   a zipformer2ctc container    the fused delegates as well (the native entries run the CTC search for such a model, k2hip.h);
//                                "greedy_search_operators" keeps the reference's unchanged CTC loops (:305-424) over OfflineProjOfHip.EncoderProj
using System;
using System.Collections.Generic;
using System.IO;
using K2TransducerAsr.Hip;
using K2TransducerAsr.Model;

namespace K2TransducerAsr
{
    // the members OfflineStream gains (partial class): on the fused route the native stream replaces `_wavFrontend` and the feature
    // buffer; Tokens / Timestamps keep their managed types and are refreshed after every GetResults / GetResult.
    public partial class OfflineStream
    {
        internal IntPtr HipStream = IntPtr.Zero;

        // what OfflineStream(OfflineCustomMetadata, int, int) (:19-35) does, without the CPU front end
        internal OfflineStream(OfflineProjOfHip proj, OfflineCustomMetadata offlineCustomMetadata)
        {
            _offlineCustomMetadata = offlineCustomMetadata;                    // :21
            _offlineInputEntity = new OfflineInputEntity();                    // :22
            _tokens = new List<Int64> { _blank_id, _blank_id };                // :34
            K2Hip.Check(K2Hip.k2hip_offline_stream_create(proj.Handle, out HipStream), "OfflineStream: create failed");
        }

        // AddSamples (:43-57) forwards here when HipStream != IntPtr.Zero -- in front of `lock (obj)`: nothing shared is touched
        internal void AddSamplesHip(float[] samples)
        {
            K2Hip.Check(K2Hip.k2hip_offline_stream_accept_samples(HipStream, samples, samples.LongLength), "AddSamples failed");
            // Speech itself never comes to the host on this route; its LENGTH is what the reference would hold (:55)
            _offlineInputEntity.SpeechLength = (int)K2Hip.k2hip_offline_stream_speech_length(HipStream);
        }

        // Samples at any rate (include/k2hip.h "Input at other sample rates"): the native stream queues them as they are and the device
        // converts the whole batch inside GetResults.  The stream's rate is fixed by its first samples; sampleRate equal to the model's is
        // AddSamples(samples).  Native streams only: the reference's CPU front end has no resampler, so a stream without one refuses.
        [System.Runtime.InteropServices.DllImport("k2hip")]
        private static extern int k2hip_offline_stream_accept_waveform(IntPtr stream, int sampleRate, float[] samples, long n);
        public void AddSamples(float[] samples, int sampleRate)
        {
            if (HipStream == IntPtr.Zero) throw new NotSupportedException("AddSamples(samples, sampleRate) needs the HIP backend");
            K2Hip.Check(k2hip_offline_stream_accept_waveform(HipStream, sampleRate, samples, samples.LongLength), "AddSamples failed");
            _offlineInputEntity.SpeechLength = (int)K2Hip.k2hip_offline_stream_speech_length(HipStream);
        }

        // Dispose(bool) (:70-91) calls this first
        internal void DisposeHip()
        {
            if (HipStream != IntPtr.Zero) { K2Hip.k2hip_offline_stream_destroy(HipStream); HipStream = IntPtr.Zero; }
        }

        // after a native GetResults / GetResult: Tokens (:292 / :180), Timestamps (:293 / :181; the native list already holds the
        // AddRange result) and the length RemoveSamples (:294, OfflineStream.cs:58-68) leaves
        internal void PullResultsHip()
        {
            int n = K2Hip.k2hip_offline_stream_num_tokens(HipStream);
            var tok = new long[n];
            K2Hip.Check(K2Hip.k2hip_offline_stream_get_tokens(HipStream, tok, n), "get_tokens failed");
            int m = K2Hip.k2hip_offline_stream_num_timestamps(HipStream);
            var ts = new int[Math.Max(m, 1)];
            K2Hip.Check(K2Hip.k2hip_offline_stream_get_timestamps(HipStream, ts, ts.Length), "get_timestamps failed");
            _tokens = new List<Int64>(tok);
            _timestamps = new List<int>(m);
            for (int i = 0; i < m; i++) _timestamps.Add(ts[i]);
            _offlineInputEntity.SpeechLength = (int)K2Hip.k2hip_offline_stream_speech_length(HipStream);
            if (_offlineInputEntity.SpeechLength == 0) _offlineInputEntity.Speech = null;
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
                int n = K2Hip.k2hip_offline_stream_num_alternatives(HipStream);
                if (n < 0) K2Hip.Check(n, "num_alternatives failed");
                return n;
            }
        }
        public Alternative GetAlternative(int i)
        {
            if (HipStream == IntPtr.Zero) throw new InvalidOperationException("GetAlternative: not a libk2hip stream");
            // the length first (no buffer is written with cap = 0 unless the alternative is empty), then the copy
            int rc = K2Hip.k2hip_offline_stream_get_alternative(HipStream, i, null, null, null, int.MaxValue, out int n, out float score);
            K2Hip.Check(rc, "get_alternative failed");
            var a = new Alternative { Tokens = new long[n], Timestamps = new int[n], TokenLogProbs = new float[n], Score = score };
            if (n > 0)
                K2Hip.Check(K2Hip.k2hip_offline_stream_get_alternative(HipStream, i, a.Tokens, a.Timestamps, a.TokenLogProbs, n, out n, out score), "get_alternative failed");
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

    public partial class OfflineRecognizer
    {
        private bool _hipSamples;   // the fused route: streams own native handles, the fbank runs on the GPU inside GetResults

        // N-best: n > 1 makes GetResults under "modified_beam_search" leave up to n alternatives, each with its token log-probs, on
        // every stream (OfflineStream.Alternatives / TokenLogProbs); 1 = off.  GetResult (the single-stream greedy path) is refused
        // natively while n > 1.
        public void SetNbest(int n)
        {
            if (!(_offlineProj is OfflineProjOfHip proj)) throw new InvalidOperationException("SetNbest: not a libk2hip recognizer");
            K2Hip.Check(K2Hip.k2hip_set_nbest(proj.Handle, n), "SetNbest failed");
        }
        public List<OfflineStream.Alternative> GetAlternatives(OfflineStream stream) { return stream.Alternatives; }

        // sherpa's lm / lm_scale for an n-gram: a text ARPA file over the token strings of tokens.txt, fused into modified_beam_search
        // (k2hip.h "n-gram LM shallow fusion"); arpaPath = null clears.  The model keeps its own copy of the scaled tables.
        public void SetNgramLm(string arpaPath, float scale)
        {
            if (!(_offlineProj is OfflineProjOfHip proj)) throw new InvalidOperationException("SetNgramLm: not a libk2hip recognizer");
            if (arpaPath == null)
            {
                K2Hip.Check(K2Hip.k2hip_set_ngram_lm(proj.Handle, IntPtr.Zero, 0f), "SetNgramLm failed");
                return;
            }
            K2Hip.Check(K2Hip.k2hip_tokens_load(_tokensFilePath, out IntPtr tokens), "SetNgramLm: tokens");
            try
            {
                K2Hip.Check(K2Hip.k2hip_ngram_lm_load(tokens, arpaPath, out IntPtr lm), "SetNgramLm: load failed");
                try { K2Hip.Check(K2Hip.k2hip_set_ngram_lm(proj.Handle, lm, scale), "SetNgramLm failed"); }
                finally { K2Hip.k2hip_ngram_lm_destroy(lm); }
            }
            finally { K2Hip.k2hip_tokens_destroy(tokens); }
        }

        // A long recording in one call (no reference counterpart; k2hip.h "Voice activity detection and long recordings"): the device cuts
        // it into segments with its voice activity detector and decodes them in batches.  One entry per segment: its range in seconds,
        // whether it was cut by force at max_speech, its token ids and their times in seconds of the recording.  The detector's level
        // defaults are untuned.  Token -> text is the caller's (DecodeMulti works on streams; these are plain id lists).
        public class LongSegment
        {
            public double StartSeconds, EndSeconds;
            public bool Forced;
            public long[] Tokens;
            public double[] TokenSeconds;
        }
        public List<LongSegment> GetResultsLong(float[] samples, int sampleRate, int maxBatch = 32, long maxBatchFrames = 32000)
        {
            if (!(_offlineProj is OfflineProjOfHip proj)) throw new InvalidOperationException("GetResultsLong: not a libk2hip recognizer");
            const double frameShift = 0.01, encoderFrame = 0.04;   // 10 ms fbank frames, subsampled by 4
            K2Hip.Check(K2Hip.k2hip_offline_recognize_long(proj.Handle, sampleRate, samples, samples.LongLength, IntPtr.Zero, maxBatch, maxBatchFrames,
                                                           out IntPtr result), "Offline recognition failed");
            try
            {
                var list = new List<LongSegment>();
                int count = K2Hip.k2hip_long_result_num_segments(result);
                for (int i = 0; i < count; i++)
                {
                    K2Hip.Check(K2Hip.k2hip_long_result_get_segment(result, i, out long start, out long end, out int forced, out int _), "GetResultsLong failed");
                    K2Hip.k2hip_long_result_get_tokens(result, i, null, null, 0, out int n);   // (the count; K2HIP_ERR_CAPACITY when n > 0)
                    var tokens = new long[n];
                    var ts = new int[n];
                    K2Hip.Check(K2Hip.k2hip_long_result_get_tokens(result, i, tokens, ts, n, out n), "GetResultsLong failed");
                    var seg = new LongSegment { StartSeconds = start * frameShift, EndSeconds = end * frameShift, Forced = forced != 0, Tokens = tokens,
                                                TokenSeconds = new double[n] };
                    for (int k = 0; k < n; k++) seg.TokenSeconds[k] = seg.StartSeconds + ts[k] * encoderFrame;
                    list.Add(seg);
                }
                return list;
            }
            finally { K2Hip.k2hip_long_result_destroy(result); }
        }

        // the constructor's early branch (see the header): everything :30-68 does, for a .k2w container
        private string _tokensFilePath;   // (SetNgramLm reads the ARPA words through the same token table)
        private void InitHip(string encoderFilePath, string decoderFilePath, string tokensFilePath, string decodingMethod, int sampleRate, int featureDim)
        {
            K2Hip.SplitSpec(encoderFilePath, decoderFilePath, out string k2wPath, out int device);
            var proj = new OfflineProjOfHip(k2wPath, device);
            _offlineProj = proj;
            _offlineModel = new OfflineModel("", "", "", 1);          // no sessions: initModel("") returns null (OfflineModel.cs:86-89)
            _offlineModel.CustomMetadata = proj.CustomMetadata;       // what :73, :95, :191, :307, :367 read
            _offlineModel.FeatureDim = featureDim;                    // :31
            _tokens = File.ReadAllLines(tokensFilePath);              // :32
            _tokensFilePath = tokensFilePath;
            _frontendConfEntity = new FrontendConfEntity();           // :34-37
            _frontendConfEntity.fs = sampleRate;
            _frontendConfEntity.n_mels = featureDim;
            _wavFrontend = new WavFrontend(_frontendConfEntity);
            bool ctc = proj.CustomMetadata.Model_type == "zipformer2ctc";   // :46-49
            switch (decodingMethod)
            {
                case "greedy_search_operators":                       // managed streams, CPU fbank, the reference's own loops
                    _hipSamples = false;
                    if (ctc)
                    {
                        _forward = new ForwardOffline(this.ForwardGreedySearchCTC);
                        _forwardBatch = new ForwardBatchOffline(this.ForwardBatchGreedySearchCTC);
                    }
                    else
                    {
                        _forward = new ForwardOffline(this.ForwardGreedySearch);
                        _forwardBatch = new ForwardBatchOffline(this.ForwardBatchGreedySearch);
                    }
                    break;
                case "modified_beam_search":
                    K2Hip.Check(K2Hip.k2hip_set_decoding_method(proj.Handle, "modified_beam_search", 4), "OfflineRecognizer: decoding method");
                    _hipSamples = true;
                    _forward = new ForwardOffline(this.ForwardGreedySearchHip);          // (the single-stream path stays greedy, k2hip.h)
                    _forwardBatch = new ForwardBatchOffline(this.ForwardBatchGreedySearchHip);
                    break;
                default:                                                                 // "greedy_search", "greedy_search_ctc", and :63-66's default
                    _hipSamples = true;
                    _forward = new ForwardOffline(this.ForwardGreedySearchHip);
                    _forwardBatch = new ForwardBatchOffline(this.ForwardBatchGreedySearchHip);
                    break;
            }
        }

        // replaces ForwardBatchGreedySearch (:189-303) -- and, for a CTC container, ForwardBatchGreedySearchCTC (:366-424): one native
        // call for the batch, from the samples the streams were given
        private void ForwardBatchGreedySearchHip(List<OfflineStream> streams)
        {
            var proj = (OfflineProjOfHip)_offlineProj;
            int B = streams.Count;
            var handles = new IntPtr[B];
            for (int i = 0; i < B; i++)
            {
                if (streams[i].HipStream == IntPtr.Zero)
                    throw new Exception("Offline recognition failed", new Exception("stream " + i + " was not created by this recognizer's CreateOfflineStream"));
                handles[i] = streams[i].HipStream;
            }
            K2Hip.Check(K2Hip.k2hip_offline_recognizer_get_results(proj.Handle, handles, B), "Offline recognition failed");   // same message as :299-302
            for (int m = 0; m < B; m++) streams[m].PullResultsHip();                  // :289-296
        }

        // replaces ForwardGreedySearch (:93-187) / ForwardGreedySearchCTC (:305-364)
        private void ForwardGreedySearchHip(OfflineStream stream)
        {
            var proj = (OfflineProjOfHip)_offlineProj;
            if (stream.HipStream == IntPtr.Zero)
                throw new Exception("Offline recognition failed", new Exception("the stream was not created by this recognizer's CreateOfflineStream"));
            K2Hip.Check(K2Hip.k2hip_offline_recognizer_get_result(proj.Handle, stream.HipStream), "Offline recognition failed");   // :183-186
            stream.PullResultsHip();                                                 // :180-181
        }
    }
}
