// Compressed block (§3.1.1.3) of a zstd frame: literals section, sequences section, sequence execution.  Included by
// zstd_frame.inc inside namespace zs.

// FSE mode of one of LL / OF / ML at in[ip, lim) (§3.1.1.3.2.2): the table in L->tab + TAB_OFF[t]
ZS_FN bool seq_table(const uint8_t* in, uint32_t& ip, uint32_t lim, int mode, int t, Lds* L, Ctl* c) {
    uint32_t* tab = L->tab + TAB_OFF[t];
    if (mode == 0) {  // predefined
        if (!fse_predefined(L, t)) return false;
        c->tab_log[t] = (uint32_t)predefined(t).log;
    } else if (mode == 1) {  // RLE: one symbol
        if (ip >= lim) return false;
        const uint32_t s = in[ip++];
        if (s > (uint32_t)TAB_MAXSYM[t]) return false;
        tab[0] = s;
        c->tab_log[t] = 0;
    } else if (mode == 2) {
        int nsym, log;
        if (!fse_header(in, ip, lim, TAB_MAXLOG[t], TAB_MAXSYM[t], L->norm, nsym, log)) return false;
        if (!fse_build(tab, L->norm, L->sdesc, nsym, log)) return false;
        c->tab_log[t] = (uint32_t)log;
    } else if (!c->tab_valid[t]) {  // repeat: the previous block's table
        return false;
    }
    c->tab_valid[t] = 1;
    return true;
}

// one literal of the block (uniform kind)
ZS_FN inline uint8_t lit_at(const uint8_t* in, const uint8_t* lit, uint32_t kind, uint32_t src, uint32_t byte, uint32_t i) {
    if (kind == 0) return in[src + i];
    if (kind == 1) return (uint8_t)byte;
    return zs_load_own(lit + i);
}

// block content in[ip, bend) -> out[c->op, ...)
ZS_FN bool decode_block(const uint8_t* __restrict__ in, uint32_t ip0, uint32_t bend, uint8_t* __restrict__ out, uint32_t n,
                             uint8_t* __restrict__ lit, Lds* L) {
    ZS_LANE_DECL;
    Ctl* c = &L->c;
    // sequence-decoder state: lane 0's alone (lives across batches)
    BitBack br;
    uint32_t sll = 0, sof = 0, sml = 0, rep0 = 0, rep1 = 0, rep2 = 0, op_s = 0, used = 0, left = 0;
    ZS_SYNC();
    ZS_SERIAL {  // literals section header (§3.1.1.3.1) and, for Huffman literals, the tree and stream layout
        c->err = 1;
        c->huf_new = 0;
        uint32_t ip = ip0;
        do {
            if (ip >= bend) break;
            const uint32_t b0 = in[ip];
            const uint32_t ltype = b0 & 3u, sf = (b0 >> 2) & 3u;
            uint32_t regen, csz = 0, nstr = 1;
            if (ltype <= 1) {
                if (sf == 0 || sf == 2) {
                    regen = b0 >> 3;
                    ip += 1;
                } else if (sf == 1) {
                    if (bend - ip < 2) break;
                    regen = (b0 >> 4) + ((uint32_t)in[ip + 1] << 4);
                    ip += 2;
                } else {
                    if (bend - ip < 3) break;
                    regen = (b0 >> 4) + ((uint32_t)in[ip + 1] << 4) + ((uint32_t)in[ip + 2] << 12);
                    ip += 3;
                }
                if (regen > BLOCK_MAX) break;
                c->lit_n = regen;
                if (ltype == 0) {
                    if (regen > bend - ip) break;
                    c->lit_kind = 0;
                    c->lit_src = ip;
                    ip += regen;
                } else {
                    if (ip >= bend) break;
                    c->lit_kind = 1;
                    c->lit_byte = in[ip];
                    ip += 1;
                }
            } else {
                const uint32_t hb = sf <= 1 ? 3u : sf + 2u;  // header bytes: 3, 3, 4, 5
                if (bend - ip < hb) break;
                uint64_t h = 0;
                for (uint32_t j = 0; j < hb; ++j) h |= (uint64_t)in[ip + j] << (8 * j);
                const int bits = sf <= 1 ? 10 : (sf == 2 ? 14 : 18);
                regen = (uint32_t)((h >> 4) & ((1u << bits) - 1));
                csz = (uint32_t)((h >> (4 + bits)) & ((1u << bits) - 1));
                nstr = sf == 0 ? 1u : 4u;
                ip += hb;
                if (regen > BLOCK_MAX || csz > bend - ip) break;
                const uint32_t lend = ip + csz;
                if (ltype == 2) {
                    if (!huf_header(in, ip, lend, L, c)) break;
                    c->huf_valid = 1;
                    c->huf_new = 1;
                } else if (!c->huf_valid) {  // treeless: the frame's previous tree
                    break;
                }
                if (nstr == 1) {
                    c->hs_off[0] = ip;
                    c->hs_len[0] = lend - ip;
                    c->hs_out[0] = 0;
                    c->hs_cnt[0] = regen;
                } else {
                    if (lend - ip < 6) break;
                    const uint32_t l1 = in[ip] | ((uint32_t)in[ip + 1] << 8), l2 = in[ip + 2] | ((uint32_t)in[ip + 3] << 8),
                                   l3 = in[ip + 4] | ((uint32_t)in[ip + 5] << 8);
                    ip += 6;
                    const uint32_t total = lend - ip;
                    if (l1 + l2 + l3 > total) break;
                    const uint32_t seg = (regen + 3) / 4;
                    if (3 * seg > regen) break;
                    c->hs_off[0] = ip;
                    c->hs_len[0] = l1;
                    c->hs_off[1] = ip + l1;
                    c->hs_len[1] = l2;
                    c->hs_off[2] = ip + l1 + l2;
                    c->hs_len[2] = l3;
                    c->hs_off[3] = ip + l1 + l2 + l3;
                    c->hs_len[3] = total - l1 - l2 - l3;
                    for (int k = 0; k < 4; ++k) {
                        c->hs_out[k] = seg * k;
                        c->hs_cnt[k] = k < 3 ? seg : regen - 3 * seg;
                    }
                }
                c->nstr = nstr;
                c->lit_kind = 2;
                c->lit_n = regen;
                ip = lend;
            }
            c->ip = ip;
            c->err = 0;
        } while (0);
    }
    ZS_SYNC();
    if (c->err) return false;
    if (c->lit_kind == 2) {
        if (c->huf_new) {  // the decode table: symbol s owns 2^(maxbits - nbits) consecutive entries from hstart[s]
            const uint32_t nsym = c->huf_nsym, mb = c->huf_bits;
            for (uint32_t s = lane; s < nsym; s += ZS_WIDTH) {
                const uint32_t w = L->hw[s];
                if (!w) continue;
                const uint32_t nb = mb + 1 - w, st = L->hstart[s], cnt = 1u << (mb - nb);
                for (uint32_t j = 0; j < cnt; ++j) L->huf[st + j] = (uint16_t)(s | (nb << 8));
            }
            ZS_SYNC();
        }
        const uint32_t nstr = c->nstr, mb = c->huf_bits;
        for (uint32_t k = lane; k < nstr; k += ZS_WIDTH) {  // one lane per Huffman stream
            BitBack hb;
            const uint32_t cnt = c->hs_cnt[k];
            uint8_t* o = lit + c->hs_out[k];
            bool ok = hb.init(in + c->hs_off[k], c->hs_len[k]);
            if (ok) {
                for (uint32_t i = 0; i < cnt; ++i) {
                    const uint32_t e = L->huf[hb.peek((int)mb)];
                    o[i] = (uint8_t)(e & 0xffu);
                    hb.off -= (int32_t)(e >> 8);
                }
                ok = hb.off == 0;
            }
            c->herr[k] = ok ? 0u : 1u;
        }
        zs_wait_own_stores();  // the literals are read back by every lane
        ZS_SYNC();
        for (uint32_t k = 0; k < nstr; ++k)
            if (c->herr[k]) return false;
    }
    ZS_SYNC();
    ZS_SERIAL {  // sequences section header (§3.1.1.3.2.1) and the tables; then the bitstream's initial states
        c->err = 1;
        uint32_t ip = c->ip;
        do {
            if (ip >= bend) break;
            uint32_t nseq = in[ip++];
            if (nseq >= 128) {
                if (nseq < 255) {
                    if (ip >= bend) break;
                    nseq = ((nseq - 128) << 8) + in[ip++];
                } else {
                    if (bend - ip < 2) break;
                    nseq = in[ip] + ((uint32_t)in[ip + 1] << 8) + 0x7f00u;
                    ip += 2;
                }
            }
            c->nseq = nseq;
            if (nseq > 0) {
                if (ip >= bend) break;
                const uint32_t modes = in[ip++];
                if (modes & 3u) break;
                if (!seq_table(in, ip, bend, (int)(modes >> 6), T_LL, L, c)) break;
                if (!seq_table(in, ip, bend, (int)((modes >> 4) & 3u), T_OF, L, c)) break;
                if (!seq_table(in, ip, bend, (int)((modes >> 2) & 3u), T_ML, L, c)) break;
                if (!br.init(in + ip, bend - ip)) break;
                sll = br.read((int)c->tab_log[T_LL]);
                sof = br.read((int)c->tab_log[T_OF]);
                sml = br.read((int)c->tab_log[T_ML]);
                if (br.off < 0) break;
            }
            c->err = 0;
        } while (0);
        op_s = c->op;
        used = 0;
        left = c->nseq;
    }
    ZS_SYNC();
    if (c->err) return false;
    const uint32_t lkind = c->lit_kind, lsrc = c->lit_src, lbyte = c->lit_byte, lit_n = c->lit_n;
    uint32_t nleft = c->nseq;
    while (nleft > 0) {
        ZS_SYNC();
        ZS_SERIAL {  // up to NB sequences (§3.1.1.3.2.2 - §3.1.2.5) into the LDS batch
            c->err = 1;
            const uint32_t nb = left < (uint32_t)NB ? left : (uint32_t)NB;
            uint32_t i = 0;
            const uint32_t* tll = L->tab + TAB_OFF[T_LL];
            const uint32_t* tof = L->tab + TAB_OFF[T_OF];
            const uint32_t* tml = L->tab + TAB_OFF[T_ML];
            rep0 = c->rep[0];  // (the repeat offsets live across the blocks of a frame)
            rep1 = c->rep[1];
            rep2 = c->rep[2];
            for (; i < nb; ++i) {
                const uint32_t el = tll[sll], eo = tof[sof], em = tml[sml];
                const uint32_t ofc = eo & 0xffu, mlc = em & 0xffu, llc = el & 0xffu;
                const uint32_t ofv = (1u << ofc) + br.read((int)ofc);
                const uint32_t ml = ML_BASE[mlc] + br.read(ML_BITS[mlc]);
                const uint32_t ll = LL_BASE[llc] + br.read(LL_BITS[llc]);
                uint32_t off;
                if (ofv > 3) {
                    off = ofv - 3;
                    rep2 = rep1;
                    rep1 = rep0;
                    rep0 = off;
                } else {
                    const uint32_t idx = ofv - 1 + (ll == 0 ? 1u : 0u);
                    if (idx == 0) {
                        off = rep0;
                    } else {
                        off = idx == 1 ? rep1 : (idx == 2 ? rep2 : rep0 - 1);
                        if (idx > 1) rep2 = rep1;
                        rep1 = rep0;
                        rep0 = off;
                    }
                }
                if (left - i > 1) {  // not the last sequence: next states (LL, ML, OF)
                    sll = (el >> 16) + br.read((int)((el >> 8) & 0xffu));
                    sml = (em >> 16) + br.read((int)((em >> 8) & 0xffu));
                    sof = (eo >> 16) + br.read((int)((eo >> 8) & 0xffu));
                }
                if (br.off < 0) break;                               // bitstream under-run
                if (ll > lit_n - used || ll > n - op_s) break;       // literals / output
                if (ml > n - op_s - ll) break;
                if (off == 0 || off > op_s + ll) break;              // before the frame's first byte
                L->b_out[i] = op_s;
                L->b_lit[i] = used;
                L->b_ll[i] = ll;
                L->b_ml[i] = ml;
                L->b_off[i] = off;
                op_s += ll + ml;
                used += ll;
            }
            c->rep[0] = rep0;
            c->rep[1] = rep1;
            c->rep[2] = rep2;
            if (i == nb) {
                left -= nb;
                c->nbatch = nb;
                c->err = 0;
                if (left == 0 && br.off != 0) c->err = 1;  // the bitstream must be consumed exactly
            }
        }
        ZS_SYNC();
        if (c->err) return false;
        const uint32_t nb = c->nbatch;
        nleft -= nb;
        {  // literals of the batch, all lanes over all of them: byte t belongs to the last sequence whose literals start <= t
            const uint32_t lit0 = L->b_lit[0], tot = L->b_lit[nb - 1] + L->b_ll[nb - 1] - lit0;
            for (uint32_t t = lane; t < tot; t += ZS_WIDTH) {
                const uint32_t q = lit0 + t;
                uint32_t lo = 0, hi = nb - 1;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi + 1) >> 1;
                    if (L->b_lit[mid] <= q) lo = mid;
                    else hi = mid - 1;
                }
                out[L->b_out[lo] + (q - L->b_lit[lo])] = lit_at(in, lit, lkind, lsrc, lbyte, q);
            }
        }
        zs_wait_own_stores();
        ZS_SYNC();
        // matches in order; a match reads output only: wait for this wave's stores when its source reaches a byte written since
        // the last wait.  A match that overlaps itself (offset < length) is periodic in its offset.
        uint32_t dirty = 0xffffffffu;
        for (uint32_t i = 0; i < nb; ++i) {
            const uint32_t p = L->b_out[i] + L->b_ll[i], ml = L->b_ml[i], off = L->b_off[i];
            const uint32_t from = p - off, span = off < ml ? off : ml;
            if (from + span > dirty) {
                zs_wait_own_stores();
                dirty = 0xffffffffu;
            }
            if (off >= ml) {
                for (uint32_t j = lane; j < ml; j += ZS_WIDTH) out[p + j] = zs_load_own(out + from + j);
            } else {
                uint32_t r = lane % off;
                const uint32_t step = ZS_WIDTH % off;
                for (uint32_t j = lane; j < ml; j += ZS_WIDTH) {
                    out[p + j] = zs_load_own(out + from + r);
                    r += step;
                    r -= r >= off ? off : 0u;
                }
            }
            if (ml > 0 && p < dirty) dirty = p;
        }
        zs_wait_own_stores();
    }
    ZS_SYNC();
    ZS_SERIAL {  // the literals after the last sequence
        c->err = 1;
        const uint32_t rest = lit_n - used;
        if (rest <= n - op_s) {
            c->tail_op = op_s;
            c->tail_lit = used;
            c->tail_n = rest;
            c->op = op_s + rest;
            c->err = 0;
        }
    }
    ZS_SYNC();
    if (c->err) return false;
    {
        const uint32_t top = c->tail_op, tl = c->tail_lit, tn = c->tail_n;
        for (uint32_t t = lane; t < tn; t += ZS_WIDTH) out[top + t] = lit_at(in, lit, lkind, lsrc, lbyte, tl + t);
    }
    return true;
}
