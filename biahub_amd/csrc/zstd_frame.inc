// Zstandard (RFC 8878) frame decoder, one wavefront per frame: the body of zstd.hip's decompress kernel.
//
// The wave's control flow is uniform.  What is serial by nature — headers, FSE and Huffman table descriptions, the sequence
// bitstream — runs on lane 0 (ZS_SERIAL) and hands its results to the other lanes through the wave's LDS record (`Lds`), always
// with ZS_SYNC (a wavefront fence and barrier) between producer and consumer.  The wide parts — Huffman table fill, literal
// copies, match copies — run on all ZS_WIDTH lanes.  The macros, `zs_wait_own_stores()` and `zs_load_own(p)` (a byte of this
// wave's own earlier global output) come from zstd_lanes.inc, which the including file brings in first: for the wavefront
// (zstd.hip's kernel) and, with one lane, for the host (bh_host_zstd_decompress: CPU tests and a host sanitizer reach the parser).
//
// Every bound is checked without overflow: input positions against the frame's csize, output positions against dlen, match
// offsets against the bytes produced so far, table logs against their RFC limits, and the backward bitstreams for under- and
// over-run.  A failure raises Ctl::err and the frame stops.

namespace zs {

#include "zstd_format.inc"

constexpr int NB = 128;                      // sequences decoded per batch
constexpr uint32_t LIT_SCRATCH = BLOCK_MAX;  // per wave: Huffman-coded literals of one block
constexpr int TAB_OFF[3] = {0, 512, 768};  // LL: 2^9 entries, OF: 2^8, ML: 2^9
constexpr int TAB_MAXLOG[3] = {9, 8, 9};
constexpr int TAB_MAXSYM[3] = {35, 31, 52};

// the wave's control record: written by lane 0, read by all lanes after ZS_SYNC
struct Ctl {
    uint32_t err, ip, op, last, content_checksum;
    uint32_t btype, bsize, src, len, rle;     // current block (raw / RLE: src, len, rle)
    uint32_t lit_kind, lit_src, lit_n, lit_byte;  // 0 raw (at in + lit_src), 1 RLE, 2 Huffman (in the scratch)
    uint32_t nstr, hs_off[4], hs_len[4], hs_out[4], hs_cnt[4], herr[4];
    uint32_t huf_valid, huf_bits, huf_nsym, huf_new;
    uint32_t tab_valid[3], tab_log[3];
    uint32_t nseq, nbatch, rep[3];
    uint32_t tail_op, tail_lit, tail_n;       // the literals after the last sequence
};

struct Lds {
    uint16_t huf[1 << HUF_MAXBITS];  // symbol | nbits << 8, indexed by the next HUF bits of the stream
    uint32_t tab[512 + 256 + 512];   // FSE decode entries: symbol | nbits << 8 | baseline << 16
    uint32_t hwtab[64];              // FSE table of the Huffman weights
    uint16_t hstart[256];            // first huf entry of each symbol
    uint8_t hw[256];                 // Huffman weights
    int16_t norm[64];
    uint16_t sdesc[64];
    uint32_t b_out[NB], b_lit[NB], b_ll[NB], b_ml[NB], b_off[NB];  // a batch of sequences
    Ctl c;
};

// backward bitstream (§4.1) over p[0, n): `off` bits remain below the cursor; bits below 0 read as zeros
struct BitBack {
    const uint8_t* p;
    uint32_t n;
    int32_t off, wlo;
    uint64_t w;
    ZS_FN bool init(const uint8_t* p_, uint32_t n_) {
        p = p_;
        n = n_;
        wlo = 1 << 30;
        w = 0;
        if (n == 0 || n > (1u << 24)) return false;
        const uint32_t last = p[n - 1];
        if (last == 0) return false;  // no end marker
        off = (int32_t)(8 * (n - 1)) + highbit(last);
        return true;
    }
    ZS_FN void reload() {
        int32_t bs = ((off + 7) >> 3) - 8;
        bs = bs < 0 ? 0 : bs;
        uint64_t v = 0;
        if ((uint32_t)bs + 8 <= n) {
            for (int j = 0; j < 8; ++j) v |= (uint64_t)p[bs + j] << (8 * j);
        } else {
            for (int j = 0; j < 8; ++j)
                if ((uint32_t)(bs + j) < n) v |= (uint64_t)p[bs + j] << (8 * j);
        }
        w = v;
        wlo = 8 * bs;
    }
    ZS_FN uint32_t peek(int k) {  // 1 <= k <= 32: bits [off - k, off)
        if (off <= 0) return 0;
        const int32_t lo = off - k;
        if (lo < wlo || off > wlo + 64) reload();
        const uint64_t mask = (1ull << k) - 1;
        if (lo >= wlo) return (uint32_t)((w >> (lo - wlo)) & mask);
        return (uint32_t)((w << (wlo - lo)) & mask);  // (wlo == 0: zeros below the stream)
    }
    ZS_FN uint32_t read(int k) {
        if (k == 0) return 0;
        const uint32_t v = peek(k);
        off -= k;
        return v;
    }
};

// k (<= 24) bits at bit `bo` of in[0, avail), LSB first; zeros beyond
ZS_FN inline uint32_t fwd_bits(const uint8_t* in, uint32_t avail, uint32_t bo, int k) {
    uint32_t v = 0;
    const uint32_t b0 = bo >> 3;
    for (int j = 0; j < 4; ++j)
        if (b0 + j < avail) v |= (uint32_t)in[b0 + j] << (8 * j);
    return (v >> (bo & 7)) & ((1u << k) - 1);
}

// FSE table description (§4.1.1) at in[ip, lim) -> norm[0, nsym), log; advances ip
ZS_FN bool fse_header(const uint8_t* in, uint32_t& ip, uint32_t lim, int maxlog, int maxsym, int16_t* norm, int& nsym, int& log) {
    if (ip >= lim) return false;
    const uint8_t* p = in + ip;
    const uint32_t avail = lim - ip;
    uint32_t bo = 0;
    log = (int)fwd_bits(p, avail, bo, 4) + 5;
    bo += 4;
    if (log > maxlog) return false;
    int remaining = (1 << log) + 1, threshold = 1 << log, bits = log + 1, s = 0;
    while (remaining > 1 && s <= maxsym) {
        const int mx = (2 * threshold - 1) - remaining;
        const int raw = (int)fwd_bits(p, avail, bo, bits);
        int v;
        if ((raw & (threshold - 1)) < mx) {
            v = raw & (threshold - 1);
            bo += bits - 1;
        } else {
            v = raw & (2 * threshold - 1);
            if (v >= threshold) v -= mx;
            bo += bits;
        }
        --v;
        remaining -= v < 0 ? -v : v;
        if (remaining < 1) return false;
        norm[s++] = (int16_t)v;
        if (v == 0) {
            int rep;
            do {
                rep = (int)fwd_bits(p, avail, bo, 2);
                bo += 2;
                if (bo > 8 * avail) return false;
                for (int i = 0; i < rep; ++i) {
                    if (s > maxsym) return false;
                    norm[s++] = 0;
                }
            } while (rep == 3);
        }
        while (remaining < threshold) {
            --bits;
            threshold >>= 1;
        }
        if (bo > 8 * avail) return false;
    }
    if (remaining != 1 || bo > 8 * avail) return false;
    nsym = s;
    ip += (bo + 7) >> 3;
    return true;
}

// decode table from normalized counts (§4.1.1): entries symbol | nbits << 8 | baseline << 16
ZS_FN bool fse_build(uint32_t* tab, const int16_t* norm, uint16_t* sdesc, int nsym, int log) {
    const uint32_t size = 1u << log;
    uint32_t total = 0;
    for (int s = 0; s < nsym; ++s) total += norm[s] < 0 ? 1u : (uint32_t)norm[s];
    if (total != size) return false;
    // sdesc[s]: the symbol's next sub-state, from its count up
    if (fse_spread(tab, norm, nsym, log, [&](int s, uint32_t n) { sdesc[s] = (uint16_t)n; }) < 0) return false;
    for (uint32_t i = 0; i < size; ++i) {
        const uint32_t s = tab[i] & 0xffu;
        const uint32_t d = sdesc[s]++;
        const int nb = log - highbit(d);
        const uint32_t base = (d << nb) - size;
        tab[i] = s | ((uint32_t)nb << 8) | (base << 16);
    }
    return true;
}

ZS_FN bool fse_predefined(Lds* L, int t) {
    const Predef p = predefined(t);
    for (int s = 0; s < p.nsym; ++s) L->norm[s] = p.norm[s];
    return fse_build(L->tab + TAB_OFF[t], L->norm, L->sdesc, p.nsym, p.log);
}

// Huffman tree description (§4.2.1) at in[ip, lim): weights -> L->hw, per-symbol table starts -> L->hstart
ZS_FN bool huf_header(const uint8_t* in, uint32_t& ip, uint32_t lim, Lds* L, Ctl* c) {
    if (ip >= lim) return false;
    const uint32_t hdr = in[ip++];
    uint32_t nw = 0;
    if (hdr >= 128) {
        nw = hdr - 127;
        const uint32_t nbytes = (nw + 1) / 2;
        if (nbytes > lim - ip) return false;
        for (uint32_t i = 0; i < nw; ++i) {
            const uint32_t b = in[ip + i / 2];
            L->hw[i] = (uint8_t)((i & 1) ? (b & 15u) : (b >> 4));
        }
        ip += nbytes;
    } else {
        if (hdr == 0 || hdr > lim - ip) return false;
        const uint32_t end = ip + hdr;
        uint32_t q = ip;
        int nsym, log;
        if (!fse_header(in, q, end, 6, 12, L->norm, nsym, log)) return false;
        if (!fse_build(L->hwtab, L->norm, L->sdesc, nsym, log)) return false;
        if (q >= end) return false;
        BitBack br;
        if (!br.init(in + q, end - q)) return false;
        uint32_t s1 = br.read(log), s2 = br.read(log);
        if (br.off < 0) return false;
        for (;;) {
            if (nw >= 255) return false;
            uint32_t e = L->hwtab[s1];
            L->hw[nw++] = (uint8_t)(e & 0xffu);
            s1 = (e >> 16) + br.read((int)((e >> 8) & 0xffu));
            if (br.off < 0) {
                L->hw[nw++] = (uint8_t)(L->hwtab[s2] & 0xffu);
                break;
            }
            if (nw >= 255) return false;
            e = L->hwtab[s2];
            L->hw[nw++] = (uint8_t)(e & 0xffu);
            s2 = (e >> 16) + br.read((int)((e >> 8) & 0xffu));
            if (br.off < 0) {
                L->hw[nw++] = (uint8_t)(L->hwtab[s1] & 0xffu);
                break;
            }
        }
        if (nw > 255) return false;
        ip = end;
    }
    uint32_t total = 0;
    for (uint32_t i = 0; i < nw; ++i) {
        if (L->hw[i] > HUF_MAXBITS) return false;
        if (L->hw[i]) total += 1u << (L->hw[i] - 1);
    }
    if (total == 0) return false;
    const int maxbits = highbit(total) + 1;
    if (maxbits > HUF_MAXBITS) return false;
    const uint32_t rest = (1u << maxbits) - total;
    if (rest & (rest - 1)) return false;  // (rest > 0: maxbits is above the highest bit of total)
    L->hw[nw] = (uint8_t)(highbit(rest) + 1);
    const uint32_t nsym = nw + 1;
    uint32_t count[HUF_MAXBITS + 2] = {0}, rank[HUF_MAXBITS + 2];
    for (uint32_t s = 0; s < nsym; ++s)
        if (L->hw[s]) ++count[maxbits + 1 - L->hw[s]];
    rank[maxbits] = 0;
    for (int i = maxbits; i >= 1; --i) rank[i - 1] = rank[i] + (count[i] << (maxbits - i));
    for (uint32_t s = 0; s < nsym; ++s) {
        if (!L->hw[s]) continue;
        const int b = maxbits + 1 - L->hw[s];
        L->hstart[s] = (uint16_t)rank[b];
        rank[b] += 1u << (maxbits - b);
    }
    c->huf_bits = (uint32_t)maxbits;
    c->huf_nsym = nsym;
    return true;
}

#include "zstd_block.inc"

// One frame: in[0, cs) -> out[0, n).  `lit`: this wave's LIT_SCRATCH bytes of global scratch.  Returns false on a corrupt frame.
ZS_FN bool decode_frame(const uint8_t* __restrict__ in, uint32_t cs, uint8_t* __restrict__ out, uint32_t n, uint8_t* __restrict__ lit,
                             Lds* L) {
    ZS_LANE_DECL;
    Ctl* c = &L->c;
    ZS_SYNC();
    ZS_SERIAL {  // frame header (§3.1.1.1)
        c->err = 1;
        c->op = 0;
        c->huf_valid = 0;
        c->rep[0] = 1;
        c->rep[1] = 4;
        c->rep[2] = 8;
        c->tab_valid[0] = c->tab_valid[1] = c->tab_valid[2] = 0;
        uint32_t ip = 0;
        do {
            if (cs < 6 || in[0] != 0x28 || in[1] != 0xb5 || in[2] != 0x2f || in[3] != 0xfd) break;
            const uint32_t fhd = in[4];
            ip = 5;
            const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1u, did_flag = fhd & 3u;
            if (fhd & 8u) break;  // reserved bit
            c->content_checksum = (fhd >> 2) & 1u;
            if (!single) ++ip;  // window descriptor: the whole frame lands in `out`, no window to keep
            const uint32_t did_bytes = did_flag == 3 ? 4u : did_flag;
            const uint32_t fcs_bytes = fcs_flag == 0 ? single : (1u << fcs_flag);
            if (did_bytes + fcs_bytes > cs - ip) break;
            uint32_t did = 0;
            for (uint32_t j = 0; j < did_bytes; ++j) did |= (uint32_t)in[ip + j] << (8 * j);
            ip += did_bytes;
            if (did != 0) break;  // dictionaries are not supported
            if (fcs_bytes) {
                uint64_t fcs = 0;
                for (uint32_t j = 0; j < fcs_bytes; ++j) fcs |= (uint64_t)in[ip + j] << (8 * j);
                if (fcs_bytes == 2) fcs += 256;
                ip += fcs_bytes;
                if (fcs != n) break;
            }
            c->ip = ip;
            c->err = 0;
        } while (0);
    }
    ZS_SYNC();
    if (c->err) return false;
    for (;;) {
        ZS_SYNC();
        ZS_SERIAL {  // block header (§3.1.1.2)
            do {
                uint32_t ip = c->ip;
                if (cs - ip < 3) { c->err = 1; break; }
                const uint32_t bh = (uint32_t)in[ip] | ((uint32_t)in[ip + 1] << 8) | ((uint32_t)in[ip + 2] << 16);
                ip += 3;
                c->last = bh & 1u;
                c->btype = (bh >> 1) & 3u;
                const uint32_t bs = bh >> 3;
                c->bsize = bs;
                const uint32_t op = c->op;
                if (c->btype == 3 || bs > BLOCK_MAX) { c->err = 1; break; }
                if (c->btype == 0) {  // raw
                    if (bs > cs - ip || bs > n - op) { c->err = 1; break; }
                    c->src = ip;
                    c->len = bs;
                    ip += bs;
                } else if (c->btype == 1) {  // RLE: one byte, bs times
                    if (ip >= cs || bs > n - op) { c->err = 1; break; }
                    c->rle = in[ip];
                    c->len = bs;
                    ip += 1;
                } else if (bs > cs - ip) {
                    c->err = 1;
                    break;
                }
                c->ip = ip;
            } while (0);
        }
        ZS_SYNC();
        if (c->err) return false;
        const uint32_t btype = c->btype;
        if (btype == 0 || btype == 1) {
            const uint32_t op = c->op, len = c->len, rle = c->rle, src = c->src;
            if (btype == 0)
                for (uint32_t j = lane; j < len; j += ZS_WIDTH) out[op + j] = in[src + j];
            else
                for (uint32_t j = lane; j < len; j += ZS_WIDTH) out[op + j] = (uint8_t)rle;
            ZS_SYNC();
            ZS_SERIAL { c->op = op + len; }
        } else {
            const uint32_t bend = c->ip + c->bsize;
            if (!decode_block(in, c->ip, bend, out, n, lit, L)) return false;
            ZS_SYNC();
            ZS_SERIAL { c->ip = bend; }
        }
        zs_wait_own_stores();  // later matches may read what this block wrote
        ZS_SYNC();
        if (c->last) break;
    }
    ZS_SERIAL {
        if (c->content_checksum && cs - c->ip < 4) c->err = 1;  // (the checksum itself is skipped)
        if (c->op != n) c->err = 1;
    }
    ZS_SYNC();
    return c->err == 0;
}

}  // namespace zs
