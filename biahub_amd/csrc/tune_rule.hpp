// Decision rule of the spectrum audition (fftconv.hip: fftconv_tune_spectrum).  Plain C++ with no HIP in it, so that a host
// program can feed it timing sequences (tests/test_tune_rule_host.py).
#pragma once

namespace bh {

struct TuneRule {
    int max_candidates;  // K: at most this many spectrum allocations are drawn and held at the same time
    float level_ratio;   // two probe times are two levels when fastest < level_ratio * slowest
};

// The default rule.  The numbers are measurements, not guesses: profiles/spectrum_audition.txt, DESIGN.md 2 ("Spectrum audition").
// K = 4: a fast block, where a process had one at all, was among its first three draws.  0.875: midway, in the log, between
// fast / slow = 0.85 and in-between / slow = 0.90, so that the early stop means the fast level is in hand.
constexpr TuneRule kTuneRuleDefault = {4, 0.875f};

struct TuneDecision {
    bool stop;  // draw no further candidate
    int keep;   // index of the candidate to keep if the audition ended here
};

// ms[0 .. n): probe time of every candidate drawn so far, in the order drawn; a value <= 0 is a candidate that failed (its
// allocation or its probe: it has no time).  The fastest timed candidate is kept (the earliest among equals; candidate 0, the
// allocation the caller came with, while nothing has a time).  The audition stops when K candidates are drawn, when the last
// one failed (memory is short or the device is in trouble: no further draws), or as soon as a fast and a slow level have both
// been seen: the fast one is then in hand.
inline TuneDecision tune_decide(const TuneRule& rule, const float* ms, int n) {
    int best = -1;
    float slowest = 0.f;
    for (int i = 0; i < n; ++i) {
        if (!(ms[i] > 0.f)) continue;
        if (best < 0 || ms[i] < ms[best]) best = i;
        if (ms[i] > slowest) slowest = ms[i];
    }
    TuneDecision d;
    d.keep = best < 0 ? 0 : best;
    d.stop = n >= rule.max_candidates || (n > 0 && !(ms[n - 1] > 0.f)) || (best >= 0 && ms[best] < rule.level_ratio * slowest);
    return d;
}

}  // namespace bh
