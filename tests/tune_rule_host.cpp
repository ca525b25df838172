// Host program of tests/test_tune_rule_host.py: feeds the audition's decision rule (biahub_amd/csrc/tune_rule.hpp) timing
// sequences the way fftconv_tune_spectrum does — one more time per draw, until the rule says stop — and prints, per case,
// where it stopped and which candidate it kept.  A sequence that runs out before the rule stops is reported with stop 0.
#include "tune_rule.hpp"

#include <cstdio>
#include <vector>

struct Case {
    const char* name;
    bh::TuneRule rule;
    std::vector<float> ms;
};

int main() {
    const bh::TuneRule r5 = {5, 0.9f};
    const std::vector<Case> cases = {
        {"one_candidate_only", {1, 0.9f}, {6.0f}},
        {"one_of_five", r5, {6.0f}},
        {"all_equal", r5, {6.0f, 6.0f, 6.0f, 6.0f, 6.0f, 6.0f, 6.0f}},
        {"fast_first", r5, {6.0f, 6.9f, 6.0f, 6.0f, 6.0f}},
        {"slow_slow_fast", r5, {6.9f, 7.0f, 6.0f, 5.0f, 5.0f}},
        {"k_reached_one_level", r5, {6.10f, 6.05f, 6.20f, 6.00f, 6.15f, 1.0f}},
        {"just_above_ratio", r5, {10.0f, 9.1f, 9.5f, 9.2f, 9.3f}},
        {"failed_second", r5, {6.0f, 0.0f, 5.0f}},
        {"failed_after_better", r5, {6.5f, 6.2f, 0.0f, 1.0f}},
        {"failed_first", r5, {0.0f, 5.0f}},
    };
    for (const Case& c : cases) {
        bh::TuneDecision d = {false, 0};
        int n = 0;
        while (!d.stop && n < (int)c.ms.size()) {
            ++n;
            d = bh::tune_decide(c.rule, c.ms.data(), n);
            if (d.keep < 0 || d.keep >= n) {
                std::printf("%s: keep %d out of range at n = %d\n", c.name, d.keep, n);
                return 1;
            }
        }
        std::printf("%s stop %d keep %d\n", c.name, d.stop ? n : 0, d.keep);
    }
    const bh::TuneRule dflt = bh::kTuneRuleDefault;
    std::printf("default K %d ratio %.4f\n", dflt.max_candidates, (double)dflt.level_ratio);
    return 0;
}
