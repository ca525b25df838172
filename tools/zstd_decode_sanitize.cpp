// The zstd frame parser (csrc/zstd_frame.inc, zstd_block.inc; host instantiation) under a host sanitizer: corrupt frames, and
// good frames cut at every length from 0 to their size, each in a heap block of exactly its length, so any read past the
// stream or write past the output is reported.  Every input must be refused or decode to the right bytes.
//   python - <<'EOF'       (from the repository root; writes the cases: u32 csize, u32 n, u32 good, frame, n expected bytes)
//   import struct, sys; sys.path[:0] = [".", "tests"]; import zstd_corpus as z
//   best = {}                                          # the smallest frame of every combination of format features
//   for fw in sorted((fw for fw in z.raw_frames() if len(fw[1]) == 32768), key=lambda fw: len(fw[0])): best.setdefault(frozenset(z.walk(fw[0])), fw)
//   good = list(best.values()) + [z.hand_frames()[k] for k in ("rle_literals", "mixed_blocks")]
//   rec = lambda f, w, g: struct.pack("<III", len(f), len(w), g) + f + w
//   open("/tmp/zstd_cases.bin", "wb").write(b"".join([rec(f, w, 0) for f, w in z.corrupt_cases()[1].values()] + [rec(f, w, 1) for f, w in good]))
//   EOF
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ibiahub_amd/csrc tools/zstd_decode_sanitize.cpp -o /tmp/zstd_decode_sanitize
//   /tmp/zstd_decode_sanitize /tmp/zstd_cases.bin
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

namespace host {
#define ZS_TARGET_HOST
#include "zstd_lanes.inc"
#include "zstd_frame.inc"
#define ZS_TARGET_END
#include "zstd_lanes.inc"
}  // namespace host

// in[0, cs) -> n bytes: 1 decoded to `want`, 0 refused, -1 accepted with other bytes
static int decode(const uint8_t* in, uint32_t cs, const uint8_t* want, uint32_t n) {
    std::unique_ptr<uint8_t[]> src(new uint8_t[cs]), dst(new uint8_t[n]), lit(new uint8_t[host::zs::LIT_SCRATCH]);
    std::unique_ptr<host::zs::Lds> lds(new host::zs::Lds);
    std::memcpy(src.get(), in, cs);
    if (!host::zs::decode_frame(src.get(), cs, dst.get(), n, lit.get(), lds.get())) return 0;
    return std::memcmp(dst.get(), want, n) == 0 ? 1 : -1;
}

int main(int argc, char** argv) {
    std::ifstream f(argc > 1 ? argv[1] : "", std::ios::binary);
    const std::vector<uint8_t> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t p = 0, cases = 0, decodes = 0, bad = 0;
    while (p + 12 <= b.size()) {
        uint32_t h[3];
        std::memcpy(h, &b[p], 12);
        const uint8_t *frame = &b[p + 12], *want = frame + h[0];
        p += 12 + (size_t)h[0] + h[1];
        if (p > b.size()) return 2;
        ++cases;
        const int whole = decode(frame, h[0], want, h[1]);
        if (whole != (int)h[2]) ++bad, std::printf("case %zu: whole frame gave %d, expected %u\n", cases, whole, h[2]);
        for (uint32_t cut = 0; h[2] && cut < h[0]; ++cut, ++decodes)
            if (decode(frame, cut, want, h[1]) < 0) ++bad, std::printf("case %zu cut at %u: accepted with wrong bytes\n", cases, cut);
    }
    std::printf("%zu cases, %zu truncated decodes, %zu failures\n", cases, decodes, bad);
    return cases == 0 || bad ? 1 : 0;
}
