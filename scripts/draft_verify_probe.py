"""Timing probe for draft verification: greedy windows of `--steps` decoder steps on seeded random weights, decoded
with the draft switch off (the yardstick) and with drafts that greedy decoding accepts to a given share, by 1, 4 and 8
concurrent callers over one window stacker; and a LocalAgreement-style growing buffer through a session view.

Method of DESIGN 26: both arms warmed up, then alternating pairs, medians.  A "window" is `decode()` of one 30 s segment:
encoder, the opening (prefill + first pick, or the verify pass) and the steps behind it.

  python scripts/draft_verify_probe.py --out profiles/draft_verify_mi355x.txt
  python scripts/draft_verify_probe.py --one-pass        # one verify pass and nothing else (for a kernel trace)
"""
import argparse
import os
import statistics
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from whisperlivekit_amd import synth, transcribe as TR                     # noqa: E402
from whisperlivekit_amd.engine import HipWhisperModel                      # noqa: E402
from whisperlivekit_amd.local_agreement import HipWhisperASR               # noqa: E402


def _round(model, mels, opts, drafts):
    """one window per caller, all callers at once -> wall seconds"""
    n = len(mels)
    gate = threading.Barrier(n + 1)
    errors = []

    def work(i):
        try:
            gate.wait()
            o = opts if drafts is None else TR.replace(opts, draft=drafts[i])
            TR.decode(model, mels[i], o)
        except BaseException as e:           # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    for t in threads:
        t.start()
    gate.wait()
    t0 = time.perf_counter()
    for t in threads:
        t.join()
    dt = time.perf_counter() - t0
    if errors:
        raise errors[0]
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="base.en")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-pass", action="store_true")
    a = ap.parse_args()
    os.environ.setdefault("WLK_SYNTHETIC_VOCAB", "1")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    model = HipWhisperModel.synthetic(a.model, 3, device=0)
    TR.set_stack(model, 8)
    eot = TR._tokenizer_for(model, "en", "transcribe").eot
    opts = TR.DecodingOptions(language="en", temperature=0.0, sample_len=a.steps, suppress_tokens=f"-1,{eot}",
                              without_timestamps=True)
    probe = model.new_session(beam=1, max_audio_seconds=1.0, batched=False)
    mels = [TR.pad_or_trim(probe.log_mel(synth.speech_like(20.0, seed=40 + i))) for i in range(8)]
    probe.close()
    truths = [TR.decode(model, m, opts).tokens for m in mels]

    def draft_of(i, share):
        d = list(truths[i])
        at = int(round(share * len(d)))
        if at < len(d):
            d[at] = 400 if d[at] != 400 else 401
        return d

    if a.one_pass:
        got = TR.decode(model, mels[0], TR.replace(opts, draft=draft_of(0, 0.9)))
        assert got.tokens == truths[0]
        TR.release_sessions(model)
        return

    say(f"# draft verification, {a.model} (seeded random weights), windows of {a.steps} decoder steps, stack=8")
    say(f"# alternating pairs ({a.pairs}) after a warm-up of both arms, medians; ms per round = all callers' windows at once")
    say("callers accepted  off_ms_round  on_ms_round  off_ms_window  on_ms_window  on/off  off_audio_s_per_s  on_audio_s_per_s")
    for callers in (1, 4, 8):
        for share in (0.0, 0.5, 0.9, 1.0):
            drafts = [draft_of(i, share) for i in range(callers)]
            # the arm gives the yardstick's tokens
            assert TR.decode(model, mels[0], TR.replace(opts, draft=drafts[0])).tokens == truths[0]
            for _ in range(2):
                _round(model, mels[:callers], opts, None)
                _round(model, mels[:callers], opts, drafts)
            off, on = [], []
            for _ in range(a.pairs):
                off.append(_round(model, mels[:callers], opts, None))
                on.append(_round(model, mels[:callers], opts, drafts))
            mo, mn = statistics.median(off) * 1e3, statistics.median(on) * 1e3
            say(f"{callers:7d} {share:8.0%} {mo:13.2f} {mn:12.2f} {mo / callers:14.2f} {mn / callers:13.2f} {mn / mo:7.3f}"
                f" {callers * 30.0 / (mo / 1e3):18.0f} {callers * 30.0 / (mn / 1e3):17.0f}")

    # ---- a growing buffer: 0.5 s per call up to 15 s, the draft is whatever the previous call produced
    say()
    say("# growing buffer: transcribe() every 0.5 s up to 15 s through a session view (word_timestamps=True, sample_len 60);")
    say("# the draft is the previous call's first window")
    audio = synth.speech_like(15.0, seed=77)
    kw = dict(temperature=0.0, sample_len=60, suppress_tokens=f"-1,{eot}", without_timestamps=True, logprob_threshold=None,
              compression_ratio_threshold=None, no_speech_threshold=None)
    accepted = []
    group = TR.window_stacker(model).group
    real_verify = group.verify

    def verify(windows, want_picks=False):
        res = real_verify(windows, want_picks)
        accepted.extend((r["accepted"], len(w[2])) for r, w in zip(res, windows))
        return res
    group.verify = verify
    ends = [int(16000 * 0.5 * i) for i in range(1, 31)]
    totals = {}
    for arm in ("off", "on", "off", "on", "off", "on"):
        asr = HipWhisperASR("en", hip_model=model, stack=8, draft=(arm == "on"))
        asr.transcribe_kargs = dict(kw)
        view = asr.session_view()
        del accepted[:]
        t0 = time.perf_counter()
        for e in ends:
            view.transcribe(audio[:e])
        totals.setdefault(arm, []).append(time.perf_counter() - t0)
    for arm in ("off", "on"):
        t = statistics.median(totals[arm][1:]) if len(totals[arm]) > 1 else totals[arm][0]
        say(f"{arm:4s} {t * 1e3:9.1f} ms for {len(ends)} calls ({t * 1e3 / len(ends):.2f} ms per call)")
    if accepted:
        say(f"verify passes {len(accepted)}, accepted {sum(k for k, _n in accepted)} of {sum(n for _k, n in accepted)} draft tokens")
    TR.release_sessions(model)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
