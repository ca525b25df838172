// Zstandard (RFC 8878) frame encoder, one wavefront per frame: the body of zstd_enc.hip's compress kernel AND of its host twin
// (bh_host_zstd_compress) — the file is included twice, once per set of the macros below.
//
// A frame is single-segment, records its content size, has no checksum and no dictionary, and holds ceil(n / 128 KiB) blocks.
// Per block: a greedy matcher (minimum match 4, offsets <= 65535, no repeat-offset codes) turns the input into sequences
// (literal length, match length, offset) and a literal buffer in per-wave global scratch, counting the literal bytes as it
// gathers them; then the literals section (Huffman with a length-limited code, 1 or 4 streams; Raw or RLE when that does not
// shrink) and the sequences section (FSE; per block and per code kind the predefined table, an RLE table or a table fitted
// to the block's codes) are written, or a Raw_Block when the block does not shrink.
//
// The wave's control flow is uniform.  What is serial by nature — Huffman code construction, the tree description (direct or
// FSE-compressed weights), the sequence bitstream, block and frame headers — runs on lane 0 (ZS_SERIAL) and exchanges its
// results with the other lanes through the wave's record (`Work`, in LDS on the device), always with ZS_SYNC between producer
// and consumer.  The wide parts run on ZS_WIDTH lanes: gathering and counting literals, ranking the symbols by count, and
// packing the Huffman streams (a prefix sum over the code lengths of ZS_WIDTH symbols gives each its bit position; the codes
// are OR-ed into a small bit buffer, whole words of which leave for the output).  The matcher's search loop is the one part
// written twice: ballot-driven on the device (the structure of lz4::compress_kernel, with its wave_extend), a plain serial loop
// on the host.
//
// The including file brings in zstd_lanes.inc first (ZS_FN, ZS_CONST, ZS_LANE_DECL, ZS_SERIAL, ZS_SYNC(), ZS_WIDTH,
// zs_scan_excl(v, &total), zs_atomic_or(p, v), zs_atomic_inc(p), zs_wait_own_stores(), zs_load_own(p)); its ZS_TARGET_DEVICE
// selects the wave-wide search loop.  Limits, tables and the FSE symbol spread are the decoder's: zstd_format.inc.
//
// Output bound.  Block k of a frame writes only inside [op_k, op_k + 3 + bs_k): its compressed body is abandoned as soon as it
// could reach bs_k bytes (every writer checks its position against `limit` first) and a Raw_Block is exactly 3 + bs_k bytes;
// op_0 is the frame header (<= 9 bytes) and op_{k+1} <= op_k + 3 + bs_k.  So a frame of n bytes never writes at or beyond
// frame_bound(n) = 9 + 3 * ceil(n / 128 KiB) + n, whether or not it is kept in the end.

namespace zse {

#include "zstd_format.inc"

constexpr int HASH_LOG = 12;
// A candidate is four equal bytes (the hash), a match is taken from ACCEPT bytes on: a sequence costs 20 to 30 bits in the
// predefined tables, more than the Huffman-coded literals a shorter match would replace (measured in DESIGN.md 3.4)
constexpr uint32_t MINMATCH = 4, ACCEPT = 6;
// a sequence covers at least ACCEPT bytes of its block, but for a match cut at the block's edge and the remainder carried in
// from the previous block (>= 3 each)
constexpr uint32_t MAXSEQ = BLOCK_MAX / ACCEPT + 8;

constexpr uint64_t frame_bound(uint64_t n) { return 9 + 3 * ((n + BLOCK_MAX - 1) / BLOCK_MAX) + n; }

enum { LIT_RAW = 0, LIT_RLE = 1, LIT_HUF = 2 };

constexpr int FSE_MAXLOG = 8;  // the largest table this encoder builds (the format allows 9 for LL and ML)
// FSE encoding table: state[cum[s] + k] is the k-th table position (ascending) of symbol s, cnt[s] its number of positions
struct FseEnc {
    uint8_t state[1 << FSE_MAXLOG];
    uint16_t cum[56], cnt[56];
    uint32_t log;
};

// written by lane 0, read by all lanes after ZS_SYNC
struct Ctl {
    uint32_t ok, op, lit_mode, nstr, lit_hdr, lit_data, tree_n;
};

struct Work {
    uint16_t table[1 << HASH_LOG];  // matcher: low 16 bits of the last position with this hash
    uint32_t hist[256];             // literal byte counts of the block
    uint32_t ncnt[512];             // Huffman tree: node weights (leaves in ascending order, then internal nodes)
    uint16_t parent[512];           // ... parent, then depth
    uint16_t order[256];            // symbols in ascending (count, symbol) order
    uint16_t code[256];
    uint8_t len[256], hw[256];      // code lengths and weights
    uint8_t tree[256];              // the tree description
    uint32_t bits[32];              // the stream packer's bit buffer
    uint32_t num[16], rank[16];
    int16_t norm[64];
    uint8_t tsym[1 << FSE_MAXLOG];
    uint16_t tnxt[56];
    FseEnc fse[4];
    Ctl c;
};

// the matcher's state across the blocks of a frame (uniform)
struct Match {
    uint32_t anchor, nl, nseq, carry_len, carry_off;
};

using blosc_frame::ld32;
using blosc_frame::st32;

// forward bit writer, least significant bit first (the FSE table description and, closed by a 1 bit, the backward streams)
struct BitW {
    uint8_t* p;
    uint32_t pos;
    uint64_t acc;
    uint32_t nb;
    ZS_FN void init(uint8_t* p_, uint32_t pos_) {
        p = p_;
        pos = pos_;
        acc = 0;
        nb = 0;
    }
    ZS_FN void add(uint32_t v, uint32_t k) {  // k <= 32, v < 2^k
        acc |= (uint64_t)v << nb;
        nb += k;
        while (nb >= 8) {
            p[pos++] = (uint8_t)acc;
            acc >>= 8;
            nb -= 8;
        }
    }
    ZS_FN void close() {  // pad with zeros to a whole byte
        if (nb) {
            p[pos++] = (uint8_t)acc;
            acc = 0;
            nb = 0;
        }
    }
};

// ---- FSE ----------------------------------------------------------------------------------------------------------------------
// the symbol spread of the decoder (fse_spread), then every symbol's positions in ascending order
ZS_FN void fse_enc_build(FseEnc* E, const int16_t* norm, int nsym, int log, uint8_t* tsym, uint16_t* tnxt) {
    uint32_t run = 0;
    // (norm sums to the table size: fse_normalize, the predefined distributions)
    fse_spread(tsym, norm, nsym, log, [&](int s, uint32_t cnt) {
        E->cum[s] = (uint16_t)run;
        E->cnt[s] = (uint16_t)cnt;
        tnxt[s] = (uint16_t)run;
        run += cnt;
    });
    for (uint32_t i = 0; i < (1u << log); ++i) E->state[tnxt[tsym[i]]++] = (uint8_t)i;
    E->log = (uint32_t)log;
}
// states are kept as table position + table size, in [size, 2 size)
ZS_FN inline uint32_t fse_first(const FseEnc* E, uint32_t s) {
    // the position whose decoder reads the most bits (sub-state cnt[s]): at least one unless the symbol owns the whole table,
    // so a decoder that ends on running out of bits does end there
    return (1u << E->log) + E->state[E->cum[s]];
}
// the state that decodes to `s` and, after reading the bits written here, continues in state x
ZS_FN inline uint32_t fse_put(const FseEnc* E, uint32_t x, uint32_t s, BitW& bw) {
    const uint32_t c = E->cnt[s];
    uint32_t nb = E->log - (uint32_t)highbit(c), d = x >> nb;
    if (d < c) {  // (then nb > 0: x >= size >= c)
        --nb;
        d = x >> nb;
    }
    bw.add(x & ((1u << nb) - 1), nb);
    return (1u << E->log) + E->state[E->cum[s] + d - c];
}

// counts cnt[0, nsym) summing to `total` -> norm[0, nsym) summing to 2^log (>= the number of present symbols): every present
// symbol at least 1, the largest takes up the difference
ZS_FN void fse_normalize(const uint32_t* cnt, int nsym, uint32_t total, int log, int16_t* norm) {
    int sum = 0;
    for (int s = 0; s < nsym; ++s) {
        int v = cnt[s] ? (int)(((uint64_t)cnt[s] << log) / total) : 0;
        if (cnt[s] && v == 0) v = 1;
        norm[s] = (int16_t)v;
        sum += v;
    }
    while (sum != (1 << log)) {
        int big = 0;
        for (int s = 1; s < nsym; ++s)
            if (norm[s] > norm[big]) big = s;
        if (sum < (1 << log)) {
            norm[big] = (int16_t)(norm[big] + (1 << log) - sum);
            sum = 1 << log;
        } else {
            --norm[big];
            --sum;
        }
    }
}
// table description (§4.1.1) of norm[0, nsym), norm[nsym - 1] != 0, no "less than 1" entries; closed to a whole byte
ZS_FN void fse_write_header(BitW& bw, const int16_t* norm, int nsym, int log) {
    bw.add((uint32_t)(log - 5), 4);
    int remaining = (1 << log) + 1, threshold = 1 << log, nbits = log + 1, s = 0;
    while (remaining > 1 && s < nsym) {
        const int v = norm[s++], mx = (2 * threshold - 1) - remaining;
        int val = v + 1;
        remaining -= v;
        if (val < mx) {
            bw.add((uint32_t)val, (uint32_t)(nbits - 1));
        } else {
            if (val >= threshold) val += mx;
            bw.add((uint32_t)val, (uint32_t)nbits);
        }
        if (v == 0) {  // the zeros that follow, three per 2-bit flag
            int z = 0;
            while (s < nsym && norm[s] == 0) {
                ++z;
                ++s;
            }
            for (; z >= 3; z -= 3) bw.add(3u, 2);
            bw.add((uint32_t)z, 2);
        }
        while (remaining < threshold) {
            --nbits;
            threshold >>= 1;
        }
    }
    bw.close();
}

// ---- Huffman ------------------------------------------------------------------------------------------------------------------
// FSE-compressed weights (§4.2.1.2) of hw[0, nw) into W->tree; false when they cannot be described in < 128 bytes
ZS_FN bool huf_weights_fse(Work* W, uint32_t nw, uint32_t* tree_n) {
    uint32_t* wc = W->num;  // how often each weight occurs
    for (int s = 0; s <= HUF_MAXBITS + 1; ++s) wc[s] = 0;
    for (uint32_t i = 0; i < nw; ++i) ++wc[W->hw[i]];
    int maxw = 0, used = 0;
    for (int s = 0; s <= HUF_MAXBITS; ++s)
        if (wc[s]) {
            maxw = s;
            ++used;
        }
    if (used < 2) return false;  // one weight only: the table description has no single-symbol form
    const int log = 6;
    fse_normalize(wc, maxw + 1, nw, log, W->norm);
    BitW bw;
    bw.init(W->tree, 1);
    fse_write_header(bw, W->norm, maxw + 1, log);
    FseEnc* E = &W->fse[T_HW];
    fse_enc_build(E, W->norm, maxw + 1, log, W->tsym, W->tnxt);
    // two interleaved states: weight i belongs to state i & 1; the last weight of each is its first state
    const int top = (int)nw - 1;
    uint32_t xa = fse_first(E, W->hw[top]), xb = fse_first(E, W->hw[top - 1]);  // xa: the state of weight `top`'s parity
    for (int i = top - 2; i >= 0; --i) {
        if ((i & 1) == (top & 1)) xa = fse_put(E, xa, W->hw[i], bw);
        else xb = fse_put(E, xb, W->hw[i], bw);
    }
    const uint32_t x0 = (top & 1) ? xb : xa, x1 = (top & 1) ? xa : xb;  // the decoder reads state 0 first: written last
    bw.add(x1 - (1u << log), (uint32_t)log);
    bw.add(x0 - (1u << log), (uint32_t)log);
    bw.add(1u, 1);
    bw.close();
    if (bw.pos - 1 >= 128) return false;
    W->tree[0] = (uint8_t)(bw.pos - 1);
    *tree_n = bw.pos;
    return true;
}

// (serial) length-limited Huffman code of the m >= 2 symbols in W->order, the tree description in W->tree, the coded bits in H
ZS_FN bool huf_build(Work* W, uint32_t m, uint32_t lastsym, uint32_t* H, uint32_t* tree_n) {
    for (uint32_t i = 0; i < m; ++i) W->ncnt[i] = W->hist[W->order[i]];
    // two queues, both ascending: the leaves and the internal nodes in the order they are made
    uint32_t li = 0, ni = m, nn = m;
    while (nn < 2 * m - 1) {
        const uint32_t a = (li < m && (ni >= nn || W->ncnt[li] <= W->ncnt[ni])) ? li++ : ni++;
        const uint32_t b = (li < m && (ni >= nn || W->ncnt[li] <= W->ncnt[ni])) ? li++ : ni++;
        W->ncnt[nn] = W->ncnt[a] + W->ncnt[b];
        W->parent[a] = W->parent[b] = (uint16_t)nn;
        ++nn;
    }
    W->parent[2 * m - 2] = 0;  // depths, root first (a parent's index is above its children's)
    for (int i = (int)(2 * m - 3); i >= 0; --i) W->parent[i] = (uint16_t)(W->parent[W->parent[i]] + 1);
    // number of codes per length, lengths beyond the limit folded into it; then codes are lengthened, one unit of the Kraft
    // sum per step, until the sum is 2^HUF_MAXBITS again: the code stays complete
    for (int l = 0; l <= HUF_MAXBITS; ++l) W->num[l] = 0;
    for (uint32_t i = 0; i < m; ++i) ++W->num[W->parent[i] < HUF_MAXBITS ? W->parent[i] : HUF_MAXBITS];
    uint32_t total = 0;
    for (int l = 1; l <= HUF_MAXBITS; ++l) total += W->num[l] << (HUF_MAXBITS - l);
    while (total > (1u << HUF_MAXBITS)) {
        --W->num[HUF_MAXBITS];
        for (int l = HUF_MAXBITS - 1; l >= 1; --l)
            if (W->num[l]) {
                --W->num[l];
                W->num[l + 1] += 2;
                break;
            }
        --total;
    }
    for (int s = 0; s < 256; ++s) W->len[s] = 0;
    uint32_t i = m;
    int maxbits = 1;
    for (int l = 1; l <= HUF_MAXBITS; ++l) {  // the most frequent symbols take the shortest codes
        for (uint32_t k = 0; k < W->num[l]; ++k) W->len[W->order[--i]] = (uint8_t)l;
        if (W->num[l]) maxbits = l;
    }
    // canonical codes as the decoder derives them: longest codes first, symbols ascending within a length
    W->rank[maxbits] = 0;
    for (int l = maxbits; l >= 1; --l) W->rank[l - 1] = W->rank[l] + (W->num[l] << (maxbits - l));
    uint32_t bits = 0;
    for (uint32_t s = 0; s <= lastsym; ++s) {
        const uint32_t l = W->len[s];
        W->hw[s] = (uint8_t)(l ? maxbits + 1 - l : 0);
        if (!l) continue;
        W->code[s] = (uint16_t)(W->rank[l] >> (maxbits - l));
        W->rank[l] += 1u << (maxbits - l);
        bits += W->hist[s] * l;
    }
    *H = bits;
    const uint32_t nw = lastsym;  // the last symbol's weight is implied
    if (nw <= 128) {              // direct 4-bit weights
        W->tree[0] = (uint8_t)(127 + nw);
        for (uint32_t k = 0; k < nw; k += 2) W->tree[1 + k / 2] = (uint8_t)((W->hw[k] << 4) | (k + 1 < nw ? W->hw[k + 1] : 0));
        *tree_n = 1 + (nw + 1) / 2;
        return true;
    }
    return huf_weights_fse(W, nw, tree_n);
}

// (wide) one Huffman stream: lits[0, cnt) coded last symbol first into dst, closed by a 1 bit; returns its bytes
ZS_FN uint32_t huf_pack(const uint8_t* lits, uint32_t cnt, uint8_t* dst, Work* W) {
    ZS_LANE_DECL;
    uint32_t pend = 0, ob = 0;  // bits waiting in W->bits, bytes written
    ZS_SYNC();
    for (uint32_t j = lane; j < 32; j += ZS_WIDTH) W->bits[j] = 0;
    ZS_SYNC();
    for (uint32_t base = 0; base < cnt; base += ZS_WIDTH) {
        const uint32_t idx = base + lane;
        uint32_t l = 0, code = 0;
        if (idx < cnt) {
            const uint32_t sym = zs_load_own(lits + (cnt - 1 - idx));
            l = W->len[sym];
            code = W->code[sym];
        }
        uint32_t total;
        const uint32_t pos = pend + zs_scan_excl(l, &total);
        if (l) {
            const uint32_t w = pos >> 5, sh = pos & 31u;
            zs_atomic_or(&W->bits[w], code << sh);
            if (sh + l > 32) zs_atomic_or(&W->bits[w + 1], code >> (32 - sh));
        }
        ZS_SYNC();
        const uint32_t tot = pend + total, nw = tot >> 5;  // (tot < 32 + 11 * ZS_WIDTH: 23 words at most)
        for (uint32_t j = lane; j < nw; j += ZS_WIDTH) st32(dst + ob + 4 * j, W->bits[j]);
        const uint32_t rest = W->bits[nw];
        ZS_SYNC();
        for (uint32_t j = lane; j <= nw; j += ZS_WIDTH) W->bits[j] = j == 0 ? rest : 0u;
        ZS_SYNC();
        ob += 4 * nw;
        pend = tot & 31u;
    }
    const uint32_t v = W->bits[0] | (1u << pend), nbytes = (pend + 8) >> 3;
    ZS_SERIAL {
        for (uint32_t j = 0; j < nbytes; ++j) dst[ob + j] = (uint8_t)(v >> (8 * j));
    }
    return ob + nbytes;
}

// ---- literals section (§3.1.1.3.1) --------------------------------------------------------------------------------------------
ZS_FN inline uint32_t raw_hdr_bytes(uint32_t nl) { return nl < 32 ? 1u : (nl < 4096 ? 2u : 3u); }
ZS_FN inline void put_raw_hdr(uint8_t* p, uint32_t type, uint32_t nl) {
    const uint32_t hb = raw_hdr_bytes(nl);
    const uint32_t v = hb == 1 ? (type | (nl << 3)) : (type | ((hb == 2 ? 1u : 3u) << 2) | (nl << 4));
    for (uint32_t j = 0; j < hb; ++j) p[j] = (uint8_t)(v >> (8 * j));
}

// (serial) choose the literals mode and write what is known of the section at out + body; c->ok = 0: the block cannot shrink
ZS_FN void plan_literals(uint8_t* out, uint32_t body, uint32_t limit, uint32_t nl, Work* W) {
    Ctl* c = &W->c;
    c->ok = 0;
    uint32_t distinct = 0, lastsym = 0;
    for (uint32_t s = 0; s < 256; ++s)
        if (W->hist[s]) {
            ++distinct;
            lastsym = s;
        }
    const uint32_t rh = raw_hdr_bytes(nl);
    uint32_t mode = LIT_RAW, sec = rh + nl, nstr = 1, hb = 0, tree_n = 0;
    if (distinct == 1) {
        mode = LIT_RLE;
        sec = rh + 1;
    } else if (distinct >= 2) {
        uint32_t H = 0;
        if (huf_build(W, distinct, lastsym, &H, &tree_n)) {
            nstr = nl < 256 ? 1u : 4u;
            hb = nl < 1024 ? 3u : (nl < 16384 ? 4u : 5u);
            // an upper bound of the section: each stream is its bits, the closing bit and padding
            const uint32_t est = hb + tree_n + (nstr == 4 ? 6u : 0u) + H / 8 + 8;
            if (est < sec) {
                mode = LIT_HUF;
                sec = est;
            }
        }
    }
    if (body + sec + 1 >= limit) return;  // with the sequence count's byte the body would not be below the block's size
    c->lit_mode = mode;
    c->nstr = nstr;
    c->lit_hdr = hb;
    c->tree_n = tree_n;
    if (mode == LIT_HUF) {
        for (uint32_t j = 0; j < tree_n; ++j) out[body + hb + j] = W->tree[j];
        c->lit_data = body + hb + tree_n + (nstr == 4 ? 6u : 0u);
    } else {
        put_raw_hdr(out + body, mode, nl);
        if (mode == LIT_RLE) out[body + rh] = (uint8_t)lastsym;
        c->lit_data = body + rh;
    }
    c->ok = 1;
}

// ---- sequences section (§3.1.1.3.2) -------------------------------------------------------------------------------------------
ZS_FN inline uint32_t ll_code(uint32_t ll) {
    if (ll < 16) return ll;
    uint32_t c = ll >= 64 ? (uint32_t)highbit(ll) + 19 : 24u;
    c = c > 35 ? 35u : c;
    while (LL_BASE[c] > ll) --c;
    return c;
}
ZS_FN inline uint32_t ml_code(uint32_t ml) {  // ml >= 3
    if (ml < 35) return ml - 3;
    uint32_t c = ml >= 131 ? (uint32_t)highbit(ml - 3) + 36 : 42u;
    c = c > 52 ? 52u : c;
    while (ML_BASE[c] > ml) --c;
    return c;
}
ZS_FN inline uint64_t seq_pack(uint32_t ll, uint32_t ml, uint32_t off) { return (uint64_t)ll | ((uint64_t)ml << 18) | ((uint64_t)off << 36); }

// (serial) the coding table of one of LL / OF / ML for this block, its description at out + pos; returns the mode (§3.1.1.3.2.1).
// cnt[0, nsym): how often each code occurs among the block's nseq sequences.  Few sequences do not pay for a description:
// Predefined_Mode; one code only: RLE_Mode; else FSE_Compressed_Mode with a table of 2^5 to 2^FSE_MAXLOG states.
ZS_FN uint32_t seq_table(Work* W, int t, const uint32_t* cnt, uint32_t nseq, uint8_t* out, uint32_t& pos) {
    FseEnc* E = &W->fse[t];
    const Predef pd = predefined(t);
    const int nmax = pd.nsym;
    int distinct = 0, last = 0;
    for (int s = 0; s < nmax; ++s)
        if (cnt[s]) {
            ++distinct;
            last = s;
        }
    if (nseq < 64) {
        for (int s = 0; s < nmax; ++s) W->norm[s] = pd.norm[s];
        fse_enc_build(E, W->norm, nmax, pd.log, W->tsym, W->tnxt);
        return 0;
    }
    if (distinct == 1) {  // a table of one state, no bits
        out[pos++] = (uint8_t)last;
        E->cum[last] = 0;
        E->cnt[last] = 1;
        E->state[0] = 0;
        E->log = 0;
        return 1;
    }
    int log = highbit(nseq) - 1;
    log = log < 5 ? 5 : (log > FSE_MAXLOG ? FSE_MAXLOG : log);
    while ((1 << log) < 2 * distinct) ++log;  // (distinct <= 53: at most 2^7)
    fse_normalize(cnt, last + 1, nseq, log, W->norm);
    BitW bw;
    bw.init(out, pos);
    fse_write_header(bw, W->norm, last + 1, log);
    pos = bw.pos;
    fse_enc_build(E, W->norm, last + 1, log, W->tsym, W->tnxt);
    return 2;
}

// (serial) the section at out + pos, never writing at or beyond `limit`; false when it does not fit
ZS_FN bool write_sequences(uint8_t* out, uint32_t& pos, uint32_t limit, const uint64_t* seqs, uint32_t nseq, Work* W) {
    // the count and the modes; from 64 sequences on (seq_table) three table descriptions of at most (4 + 53 * 9 + 53 * 2) / 8
    // < 75 bytes each
    if (pos + 4 + (nseq < 64 ? 0u : 3u * 75u) > limit) return false;
    if (nseq < 128) {
        out[pos++] = (uint8_t)nseq;
    } else if (nseq < 0x7f00u) {
        out[pos++] = (uint8_t)((nseq >> 8) + 128);
        out[pos++] = (uint8_t)nseq;
    } else {  // (not reached while MAXSEQ < 0x7f00: kept so that the header is right for any ACCEPT)
        out[pos++] = 255;
        out[pos++] = (uint8_t)(nseq - 0x7f00u);
        out[pos++] = (uint8_t)((nseq - 0x7f00u) >> 8);
    }
    if (nseq == 0) return true;
    // how often each code occurs (the literal counts are no longer needed: W->hist is free)
    uint32_t *cll = W->hist, *cof = W->hist + 64, *cml = W->hist + 128;
    for (int s = 0; s < 192; ++s) W->hist[s] = 0;
    for (uint32_t i = 0; i < nseq; ++i) {
        const uint64_t q = seqs[i];
        ++cll[ll_code((uint32_t)(q & 0x3ffffu))];
        ++cml[ml_code((uint32_t)((q >> 18) & 0x3ffffu))];
        ++cof[highbit((uint32_t)(q >> 36) + 3)];
    }
    const uint32_t mpos = pos++;
    const uint32_t mll = seq_table(W, T_LL, cll, nseq, out, pos), mof = seq_table(W, T_OF, cof, nseq, out, pos),
                   mml = seq_table(W, T_ML, cml, nseq, out, pos);
    out[mpos] = (uint8_t)((mll << 6) | (mof << 4) | (mml << 2));
    const FseEnc *ELL = &W->fse[T_LL], *EOFF = &W->fse[T_OF], *EML = &W->fse[T_ML];
    BitW bw;
    bw.init(out, pos);
    uint32_t xll = 0, xof = 0, xml = 0;
    // the decoder reads backwards: the last sequence is written first, and within a sequence the reverse of the reading
    // order (offset, match length, literal length extra bits; then the LL, ML, OF state updates)
    for (uint32_t i = nseq; i-- > 0;) {
        if (bw.pos + 16 > limit) return false;  // (a sequence adds at most 3 * (8 + 16) bits to fewer than 8 waiting)
        const uint64_t q = seqs[i];
        const uint32_t ll = (uint32_t)(q & 0x3ffffu), ml = (uint32_t)((q >> 18) & 0x3ffffu), ofv = (uint32_t)(q >> 36) + 3;
        const uint32_t llc = ll_code(ll), mlc = ml_code(ml), ofc = (uint32_t)highbit(ofv);
        if (i == nseq - 1) {
            xll = fse_first(ELL, llc);
            xof = fse_first(EOFF, ofc);
            xml = fse_first(EML, mlc);
        } else {
            xof = fse_put(EOFF, xof, ofc, bw);
            xml = fse_put(EML, xml, mlc, bw);
            xll = fse_put(ELL, xll, llc, bw);
        }
        bw.add(ll - LL_BASE[llc], LL_BITS[llc]);
        bw.add(ml - ML_BASE[mlc], ML_BITS[mlc]);
        bw.add(ofv - (1u << ofc), ofc);
    }
    if (bw.pos + 16 > limit) return false;
    bw.add(xml - (1u << EML->log), EML->log);
    bw.add(xof - (1u << EOFF->log), EOFF->log);
    bw.add(xll - (1u << ELL->log), ELL->log);
    bw.add(1u, 1);
    bw.close();
    pos = bw.pos;
    return true;
}

// ---- one block ----------------------------------------------------------------------------------------------------------------
// (wide) cnt bytes of the input become literals: copied to the scratch and counted
ZS_FN inline void gather(const uint8_t* src, uint32_t cnt, uint8_t* dst, Work* W) {
    ZS_LANE_DECL;
    for (uint32_t j = lane; j < cnt; j += ZS_WIDTH) {
        const uint8_t b = src[j];
        dst[j] = b;
        zs_atomic_inc(&W->hist[b]);
    }
}

ZS_FN inline void emit_seq(const uint8_t* in, uint32_t mp, uint32_t len, uint32_t off, uint8_t* lits, uint64_t* seqs, Match& m, Work* W) {
    ZS_LANE_DECL;
    const uint32_t lit = mp - m.anchor;
    gather(in + m.anchor, lit, lits + m.nl, W);
    ZS_SERIAL { seqs[m.nseq] = seq_pack(lit, len, off); }
    ++m.nseq;
    m.nl += lit;
    m.anchor = mp + len;
}

// a match of `len` bytes at mp, `off` back: cut at the block's edge, the remainder is carried into the next block.  A piece
// below 3 bytes (the format's shortest match) stays literals.  Returns the position behind the match, at most bend.
ZS_FN inline uint32_t take_match(const uint8_t* in, uint32_t mp, uint32_t len, uint32_t off, uint32_t bend, uint8_t* lits, uint64_t* seqs,
                                 Match& m, Work* W) {
    if (mp + len > bend) {
        m.carry_len = mp + len - bend;
        m.carry_off = off;
        len = bend - mp;
    }
    if (len >= 3) emit_seq(in, mp, len, off, lits, seqs, m, W);
    return mp + len;
}

// the block in[start, bend) of the frame in[0, n) -> sequences and literals
ZS_FN void match_block(const uint8_t* in, uint32_t n, uint32_t start, uint32_t bend, uint8_t* lits, uint64_t* seqs, Match& m, Work* W) {
    ZS_LANE_DECL;
    ZS_SYNC();
    for (uint32_t s = lane; s < 256; s += ZS_WIDTH) W->hist[s] = 0;
    ZS_SYNC();
    m.nl = 0;
    m.nseq = 0;
    m.anchor = start;
    uint32_t ip = start;
    if (m.carry_len >= 3) {  // the rest of the previous block's last match: a sequence without literals
        const uint32_t len = m.carry_len < bend - start ? m.carry_len : bend - start;
        m.carry_len -= len;
        emit_seq(in, start, len, m.carry_off, lits, seqs, m, W);
        ip = start + len;
    } else {
        m.carry_len = 0;
    }
    unsigned short* table = W->table;
#ifdef ZS_TARGET_DEVICE
    while (ip < bend && m.nseq < MAXSEQ) {  // 64 positions per step
        const uint32_t p = ip + lane;
        const bool valid = p < bend && p + 4 <= n;
        const uint32_t v = valid ? ld32(in + p) : 0u;
        const uint32_t h = (v * 2654435761u) >> (32 - HASH_LOG);
        const uint32_t e = table[h];
        if (valid) table[h] = (unsigned short)p;  // reads of the step come before its writes (a wavefront's LDS operations execute in order)
        // the position with these low 16 bits in (p - 65536, p]: distance 0 and distances beyond the frame's start fail
        const uint32_t dist = (p - e) & 0xffffu;
        // A byte run first: the bytes one back.  The table is read before the step's 64 positions enter it, so it cannot see
        // a match inside the window, and what it holds for a run's hash is the END of an earlier run of that byte, a match of
        // four: the run candidate must not be shadowed by it.
        const bool run = valid && p >= 1u && ld32(in + (p >= 1u ? p - 1 : 0u)) == v;
        const uint32_t cand = run ? p - 1 : p - dist;
        bool ok = run || (valid && dist != 0u && dist <= p);
        ok = ok && (run || ld32(in + (ok ? cand : 0u)) == v);
        unsigned long long mask = __ballot(ok);
        const uint32_t wend = ip + 64;
        uint32_t next_ip = wend;
        while (mask != 0ull) {  // every match of the window in turn
            const int first = __builtin_ctzll(mask);
            const uint32_t mp = ip + first;
            const uint32_t mc = (uint32_t)__builtin_amdgcn_readlane((int)cand, first);
            const uint32_t len = blosc_frame::wave_extend(in, mp, mc, n, (int)lane);  // to the end of the frame
            if (len < ACCEPT) {  // too short to pay for a sequence: the next candidate of the window
                mask &= mask - 1;
                continue;
            }
            const uint32_t end = take_match(in, mp, len, mp - mc, bend, lits, seqs, m, W);
            if (end >= wend || m.nseq >= MAXSEQ) {
                next_ip = end;
                break;
            }
            mask &= ~0ull << (end - ip);  // the lanes behind this match
        }
        ip = next_ip;
    }
#else
    while (ip < bend && ip + 4 <= n && m.nseq < MAXSEQ) {
        const uint32_t v = ld32(in + ip);
        const uint32_t h = (v * 2654435761u) >> (32 - HASH_LOG);
        const uint32_t e = table[h];
        table[h] = (unsigned short)ip;
        const uint32_t dist = (ip - e) & 0xffffu, cand = ip - dist;
        if (dist != 0u && dist <= ip && ld32(in + cand) == v) {
            uint32_t len = MINMATCH;
            while (ip + len < n && in[ip + len] == in[cand + len]) ++len;
            if (len >= ACCEPT) {
                ip = take_match(in, ip, len, dist, bend, lits, seqs, m, W);
                continue;
            }
        }
        ++ip;
    }
#endif
    gather(in + m.anchor, bend - m.anchor, lits + m.nl, W);  // the literals after the last sequence
    m.nl += bend - m.anchor;
    m.anchor = bend;
}

// the block's sequences and literals -> out + op: a Compressed_Block, or a Raw_Block of in[start, start + bs) when that is
// not smaller.  Writes inside [op, op + 3 + bs) only.
ZS_FN void encode_block(const uint8_t* in, uint32_t start, uint32_t bs, bool last, uint8_t* out, uint32_t& op, const uint8_t* lits,
                        uint32_t nl, const uint64_t* seqs, uint32_t nseq, Work* W) {
    ZS_LANE_DECL;
    Ctl* c = &W->c;
    const uint32_t body = op + 3, limit = body + bs;
    zs_wait_own_stores();  // the literals are read back by other lanes
    ZS_SYNC();
    for (uint32_t s = lane; s < 256; s += ZS_WIDTH) {  // rank the present symbols by (count, symbol)
        const uint32_t cs = W->hist[s];
        if (!cs) continue;
        uint32_t r = 0;
        for (uint32_t t = 0; t < 256; ++t) {
            const uint32_t ct = W->hist[t];
            r += (ct && (ct < cs || (ct == cs && t < s))) ? 1u : 0u;
        }
        W->order[r] = (uint16_t)s;
    }
    ZS_SYNC();
    ZS_SERIAL { plan_literals(out, body, limit, nl, W); }
    ZS_SYNC();
    if (c->ok) {
        const uint32_t mode = c->lit_mode, nstr = c->nstr, data = c->lit_data;
        uint32_t sb[4] = {0, 0, 0, 0};
        if (mode == LIT_RAW) {
            for (uint32_t j = lane; j < nl; j += ZS_WIDTH) out[data + j] = zs_load_own(lits + j);
        } else if (mode == LIT_HUF) {
            const uint32_t seg = nstr == 4 ? (nl + 3) / 4 : nl;
            uint32_t at = data;
            for (uint32_t k = 0; k < nstr; ++k) {
                sb[k] = huf_pack(lits + seg * k, k < 3 && nstr == 4 ? seg : nl - seg * k, out + at, W);
                at += sb[k];
            }
        }
        ZS_SYNC();
        ZS_SERIAL {
            uint32_t pos;
            if (mode == LIT_HUF) {
                const uint32_t hb = c->lit_hdr, tree_n = c->tree_n;
                const uint32_t csz = tree_n + (nstr == 4 ? 6u : 0u) + sb[0] + sb[1] + sb[2] + sb[3];
                const uint32_t sf = nstr == 1 ? 0u : hb - 2, fbits = hb == 3 ? 10u : (hb == 4 ? 14u : 18u);
                const uint64_t h = 2u | (sf << 2) | ((uint64_t)nl << 4) | ((uint64_t)csz << (4 + fbits));
                for (uint32_t j = 0; j < hb; ++j) out[body + j] = (uint8_t)(h >> (8 * j));
                if (nstr == 4)
                    for (uint32_t k = 0; k < 3; ++k) {
                        out[body + hb + tree_n + 2 * k] = (uint8_t)sb[k];
                        out[body + hb + tree_n + 2 * k + 1] = (uint8_t)(sb[k] >> 8);
                    }
                pos = body + hb + csz;
            } else {
                pos = data + (mode == LIT_RAW ? nl : 1u);
            }
            const bool fit = write_sequences(out, pos, limit, seqs, nseq, W);
            if (fit && pos - body < bs) {
                const uint32_t bh = ((pos - body) << 3) | (2u << 1) | (last ? 1u : 0u);
                out[op] = (uint8_t)bh;
                out[op + 1] = (uint8_t)(bh >> 8);
                out[op + 2] = (uint8_t)(bh >> 16);
                c->op = pos;
            } else {
                c->ok = 0;
            }
        }
        ZS_SYNC();
    }
    if (c->ok) {
        op = c->op;
        return;
    }
    ZS_SERIAL {  // Raw_Block
        const uint32_t bh = (bs << 3) | (last ? 1u : 0u);
        out[op] = (uint8_t)bh;
        out[op + 1] = (uint8_t)(bh >> 8);
        out[op + 2] = (uint8_t)(bh >> 16);
    }
    for (uint32_t j = lane; j < bs; j += ZS_WIDTH) out[body + j] = in[start + j];
    op = body + bs;
}

// One frame: in[0, n) -> out[0, returned size), n >= 1; `out` holds frame_bound(n) bytes, `lits` BLOCK_MAX bytes, `seqs`
// MAXSEQ entries.  A result >= n means "does not shrink": the content
// of `out` is then unspecified and the caller stores the input as it is.
ZS_FN uint32_t encode_frame(const uint8_t* in, uint32_t n, uint8_t* out, uint8_t* lits, uint64_t* seqs, Work* W) {
    ZS_LANE_DECL;
    ZS_SYNC();
    // (a reset table makes the frame a function of its input alone; an entry is a candidate like any other, verified by bytes)
    for (uint32_t j = lane; j < (1u << HASH_LOG); j += ZS_WIDTH) W->table[j] = 0;
    const uint32_t fcs = n < 256 ? 0u : (n < 65792u ? 1u : 2u), hdr = 5 + (fcs == 0 ? 1u : (fcs == 1 ? 2u : 4u));
    ZS_SERIAL {  // frame header (§3.1.1.1): single segment, content size, no checksum, no dictionary
        out[0] = 0x28;
        out[1] = 0xb5;
        out[2] = 0x2f;
        out[3] = 0xfd;
        out[4] = (uint8_t)((fcs << 6) | 0x20u);
        const uint32_t v = fcs == 1 ? n - 256 : n;
        for (uint32_t j = 0; j < hdr - 5; ++j) out[5 + j] = (uint8_t)(v >> (8 * j));
    }
    uint32_t op = hdr;
    Match m = {0, 0, 0, 0, 0};
    for (uint32_t start = 0; start < n; start += BLOCK_MAX) {
        const uint32_t bend = n - start < BLOCK_MAX ? n : start + BLOCK_MAX;
        match_block(in, n, start, bend, lits, seqs, m, W);
        encode_block(in, start, bend - start, bend == n, out, op, lits, m.nl, seqs, m.nseq, W);
        if (op >= n) return n;
    }
    return op;
}

}  // namespace zse
