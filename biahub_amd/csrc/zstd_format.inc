// The core of the Zstandard format (RFC 8878) shared by the frame decoder (zstd_frame.inc) and the frame encoder
// (zstd_enc.inc): limits, constant tables and the FSE symbol spread.  Included inside their namespaces, under the macros of
// zstd_lanes.inc.

constexpr uint32_t BLOCK_MAX = 128u * 1024u;
constexpr int HUF_MAXBITS = 11;
enum { T_LL = 0, T_OF = 1, T_ML = 2, T_HW = 3 };  // literal lengths, offsets, match lengths; Huffman weights

ZS_FN inline int highbit(uint32_t v) { return 31 - __builtin_clz(v); }  // v > 0

// Predefined distributions (RFC 8878 §3.1.1.3.2.2); -1 is a "less than 1" probability.  Sums with -1 as 1: 64, 64, 32.
ZS_CONST int8_t LL_NORM[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1,
                               -1, -1, -1, -1};
ZS_CONST int8_t ML_NORM[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                               1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
ZS_CONST int8_t OF_NORM[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
// literal length and match length codes: baseline and extra bits (§3.1.1.3.2.1)
ZS_CONST uint32_t LL_BASE[36] = {0,  1,  2,  3,  4,  5,  6,  7,  8,   9,   10,  11,  12,   13,   14,   15,    16,    18,
                                 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
ZS_CONST uint8_t LL_BITS[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12,
                                13, 14, 15, 16};
ZS_CONST uint32_t ML_BASE[53] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16,  17,  18,   19,   20,
                                 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,  35,  37,   39,   41,
                                 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
ZS_CONST uint8_t ML_BITS[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

// the predefined table of T_LL / T_OF / T_ML: its distribution, symbol count and log
struct Predef { const int8_t* norm; int nsym, log; };
ZS_FN inline Predef predefined(int t) { return t == T_LL ? Predef{LL_NORM, 36, 6} : (t == T_OF ? Predef{OF_NORM, 29, 5} : Predef{ML_NORM, 53, 6}); }

// The symbol spread of an FSE table of 2^log positions (§4.1.1): sym[position] = symbol.  "Less than 1" symbols take one position
// each from the top downwards, the others their norm[s] positions along the walk of (size >> 1) + (size >> 3) + 3 that skips
// the top.  each(s, n) is told every symbol in ascending order with the number of its positions (0: absent): where the two
// table builders differ.  Returns `high`, the first top position, or -1 when the walk does not come back to position 0.  The
// counts must not exceed the table (the caller's check): a walk over a full table would not end.
template <typename S, class F>
ZS_FN int32_t fse_spread(S* sym, const int16_t* norm, int nsym, int log, F each) {
    const uint32_t size = 1u << log, step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    uint32_t high = size, pos = 0;
    for (int s = 0; s < nsym; ++s)
        if (norm[s] == -1) sym[--high] = (S)s;
    for (int s = 0; s < nsym; ++s) {
        each(s, norm[s] < 0 ? 1u : (uint32_t)norm[s]);
        if (norm[s] <= 0) continue;
        for (int i = 0; i < norm[s]; ++i) {
            sym[pos] = (S)s;
            do pos = (pos + step) & mask;
            while (pos >= high);
        }
    }
    return pos == 0 ? (int32_t)high : -1;
}
