// bsx_meth_parse.h — the host-side file parsers of the methylation-ratio tool (bsx_meth.hip): BSP / SAM lines, BAM records
// out of BGZF blocks, the reference FASTA.  Plain C++ and zlib, no HIP: tests/harness/meth_parse_check.cpp builds it under
// AddressSanitizer + UndefinedBehaviorSanitizer and feeds it well-formed and hostile files (tests/test_meth_parse_cpu.py).
// Every reader here bounds-checks a field before it reads it and answers a malformed file with an error code, never
// with a read outside its buffers.
#pragma once
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "bsx_cpus.h"

namespace bsx_meth_parse {

typedef unsigned long long u64;

struct ParsedChunk {
    std::vector<uint32_t> chr; std::vector<int64_t> pos, cut; std::vector<uint8_t> strand; std::vector<int32_t> insert;
    std::vector<char> seq; std::vector<u64> off{0};
    u64 lines = 0;
    int bad = 0;
};

inline bool field(const char *&p, const char *e, const char *&b, size_t &n)  // next tab-separated column of the line [p, e)
{
    if (p > e) return false;
    b = p;
    const char *t = (const char *)memchr(p, '\t', (size_t)(e - p));
    if (!t) { n = (size_t)(e - p); p = e + 1; }
    else { n = (size_t)(t - p); p = t + 1; }
    return true;
}

// get_alignment's filters (methratio.py:31-48) for the lines of [b, e)
inline void parse_chunk(const char *b, const char *e, int sam, const std::unordered_map<std::string, uint32_t> &cid, int unique, int pair, ParsedChunk &o)
{
    std::string key;
    while (b < e) {
        const char *nl = (const char *)memchr(b, '\n', (size_t)(e - b));
        const char *le = nl ? nl : e;  // line without its newline
        const char *p = b;
        b = nl ? nl + 1 : e;
        o.lines++;
        const char *c[12]; size_t n[12];
        int nc = 0;
        while (nc < 12 && field(p, le, c[nc], n[nc])) nc++;
        if (sam) {
            if (n[0] && c[0][0] == '@') { o.lines--; continue; }
            if (nc < 11) { o.bad = 1; continue; }
            const long flag = strtol(std::string(c[1], n[1]).c_str(), nullptr, 10);
            if ((flag & 0x4) || (unique && (flag & 0x100)) || (pair && !(flag & 0x2))) continue;
            key.assign(c[2], n[2]);
            auto it = cid.find(key);
            if (it == cid.end()) continue;
            const long long pos = strtoll(std::string(c[3], n[3]).c_str(), nullptr, 10) - 1, insert = strtoll(std::string(c[8], n[8]).c_str(), nullptr, 10);
            // strand from the first ZS:Z: tag among the optional fields
            const char *q = c[10] + n[10] + 1;
            int st = -1;
            while (q <= le) {
                const char *fb; size_t fn;
                if (!field(q, le, fb, fn)) break;
                if (fn >= 7 && memcmp(fb, "ZS:Z:", 5) == 0) { st = (fb[5] == '-' ? 1 : 0) | (fb[6] == '-' ? 2 : 0); break; }
            }
            if (st < 0) { o.bad = 2; continue; }
            o.chr.push_back(it->second); o.pos.push_back(pos); o.strand.push_back((uint8_t)st); o.insert.push_back((int32_t)insert);
            o.cut.push_back(insert > 0 ? strtoll(std::string(c[7], n[7]).c_str(), nullptr, 10) - 1 : -1);
            o.seq.insert(o.seq.end(), c[9], c[9] + n[9]); o.off.push_back(o.seq.size());
        } else {
            if (nc < 4) { o.bad = 1; continue; }
            const char f0 = n[3] > 0 ? c[3][0] : 0, f1 = n[3] > 1 ? c[3][1] : 0;
            if ((f0 == 'N' && f1 == 'M') || (f0 == 'Q' && f1 == 'C')) continue;
            if (unique && !(f0 == 'U' && f1 == 'M')) continue;
            if (nc < 8) { o.bad = 1; continue; }
            if (pair && n[7] == 1 && c[7][0] == '0') continue;
            key.assign(c[4], n[4]);
            auto it = cid.find(key);
            if (it == cid.end()) continue;
            if (n[6] < 2) { o.bad = 2; continue; }
            o.chr.push_back(it->second); o.pos.push_back(strtoll(std::string(c[5], n[5]).c_str(), nullptr, 10) - 1);
            o.strand.push_back((uint8_t)((c[6][0] == '-' ? 1 : 0) | (c[6][1] == '-' ? 2 : 0)));
            o.insert.push_back((int32_t)strtoll(std::string(c[7], n[7]).c_str(), nullptr, 10)); o.cut.push_back(-1);
            o.seq.insert(o.seq.end(), c[1], c[1] + n[1]); o.off.push_back(o.seq.size());
        }
    }
}

// A BSP or SAM text file: pieces of ~`piece` bytes (bounded host memory; 256 MB in the library), each cut into per-thread
// chunks at line starts and parsed in parallel; the chunks of a piece are joined in file order and handed to `flush`
// (first-wins duplicate removal depends on that order).  Returns 0, 2 for a line without strand information, or flush's code.
template <class Flush>
int stream_text(const char *base, size_t len, int sam, const std::unordered_map<std::string, uint32_t> &cid, int unique, int pair, size_t piece, u64 &lines,
                Flush &&flush)
{
    for (size_t p0 = 0; p0 < len;) {
        size_t p1 = piece < len - p0 ? p0 + piece : len;
        if (p1 < len) { const char *nl = (const char *)memchr(base + p1, '\n', len - p1); p1 = nl ? (size_t)(nl - base) + 1 : len; }
        const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(32u, std::max(1u, bsx_usable_cpus())), (p1 - p0) / (1u << 20) + 1));
        std::vector<size_t> cut(nt + 1, p1);
        cut[0] = p0;
        for (unsigned t = 1; t < nt; t++) {
            const size_t g = p0 + (p1 - p0) * t / nt;
            const char *nl = (const char *)memchr(base + g, '\n', p1 - g);
            cut[t] = nl ? (size_t)(nl - base) + 1 : p1;
        }
        std::vector<ParsedChunk> pc(nt);
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; t++) th.emplace_back([&, t] { parse_chunk(base + cut[t], base + cut[t + 1], sam, cid, unique, pair, pc[t]); });
        parse_chunk(base + cut[0], base + cut[1], sam, cid, unique, pair, pc[0]);
        for (std::thread &x : th) x.join();
        ParsedChunk all;
        int bad = 0;
        for (ParsedChunk &q : pc) {
            if (q.bad == 2) bad = 2;
            lines += q.lines;
            const u64 b0 = all.seq.size();
            all.chr.insert(all.chr.end(), q.chr.begin(), q.chr.end()); all.pos.insert(all.pos.end(), q.pos.begin(), q.pos.end());
            all.cut.insert(all.cut.end(), q.cut.begin(), q.cut.end()); all.strand.insert(all.strand.end(), q.strand.begin(), q.strand.end());
            all.insert.insert(all.insert.end(), q.insert.begin(), q.insert.end()); all.seq.insert(all.seq.end(), q.seq.begin(), q.seq.end());
            for (size_t i = 1; i < q.off.size(); i++) all.off.push_back(b0 + q.off[i]);
        }
        if (bad) return bad;
        if (!all.chr.empty()) { const int rc = flush(all); if (rc) return rc; }
        p0 = p1;
    }
    return 0;
}

// BAM, streamed: the BGZF blocks are inflated (in parallel) a bounded window at a time — a whole-genome BAM is hundreds of GB
// inflated — and the alignment records of each window are handed to `flush` in file order (first-wins duplicate removal
// depends on it); a record, or the header, that straddles the window edge is carried into the next window.  Fields as
// `samtools view -X` would print them (what the reference reads): flag bits, RNAME from the header, POS, PNEXT, TLEN, SEQ, ZS:Z.
// Every length field is checked against what is left of its block, header or record before anything behind it is read;
// returns 1 for a file that is not a well-formed BAM, flush's code if that is not 0.
template <class Flush>
int stream_bam(const char *base, size_t len, const std::unordered_map<std::string, uint32_t> &cid, int unique, int pair, size_t window, u64 &lines, int &bad_records,
               Flush &&flush)
{
    struct Blk { size_t in_off, in_len, out_len; };
    std::vector<Blk> blks;
    size_t p = 0;
    const unsigned char *u = (const unsigned char *)base;
    while (p + 18 <= len) {
        if (u[p] != 0x1f || u[p + 1] != 0x8b || u[p + 2] != 8 || !(u[p + 3] & 4)) return 1;
        const unsigned xlen = u[p + 10] | (u[p + 11] << 8);
        if ((size_t)12 + xlen + 8 > len - p) return 1;  // the extra field and the trailer must lie inside the file
        unsigned bsize = 0;
        for (unsigned x = 0; x + 4 <= xlen;) {
            const unsigned char *f = u + p + 12 + x;
            const unsigned slen = f[2] | (f[3] << 8);
            if (x + 4 + slen > xlen) return 1;  // a subfield that runs past the extra field
            if (f[0] == 'B' && f[1] == 'C' && slen == 2) bsize = (f[4] | (f[5] << 8)) + 1;
            x += 4 + slen;
        }
        if (bsize < 12 + xlen + 8 || bsize > len - p) return 1;
        const unsigned isize = u[p + bsize - 4] | (u[p + bsize - 3] << 8) | (u[p + bsize - 2] << 16) | ((unsigned)u[p + bsize - 1] << 24);
        if (isize > 65536) return 1;  // a BGZF block holds at most 64 KB: a format error, not a reason to allocate
        blks.push_back(Blk{p + 12 + xlen, bsize - 12 - xlen - 8, isize});
        p += bsize;
    }
    auto rd32 = [](const unsigned char *q) { int32_t v; memcpy(&v, q, 4); return v; };
    static const char nt16[] = "=ACMGRSVTWYHKDBN";
    std::vector<unsigned char> buf;
    std::vector<int64_t> ref_id;  // BAM reference index -> our chromosome id or -1
    int32_t n_ref = 0;
    bool header_done = false;
    size_t carry = 0;
    for (size_t bi = 0; bi < blks.size();) {
        size_t bj = bi, out = 0;
        while (bj < blks.size() && (bj == bi || out + blks[bj].out_len <= window)) { out += blks[bj].out_len; bj++; }
        buf.resize(carry + out + 8);
        {
            std::vector<size_t> at(bj - bi + 1, carry);
            for (size_t i = bi; i < bj; i++) at[i - bi + 1] = at[i - bi] + blks[i].out_len;
            std::atomic<size_t> next(bi);
            std::atomic<int> bad(0);
            auto work = [&] {
                for (size_t i; (i = next.fetch_add(1)) < bj;) {
                    if (!blks[i].out_len) continue;
                    z_stream z;
                    memset(&z, 0, sizeof(z));
                    if (inflateInit2(&z, -15) != Z_OK) { bad = 1; continue; }
                    z.next_in = const_cast<unsigned char *>(u + blks[i].in_off); z.avail_in = (unsigned)blks[i].in_len;
                    z.next_out = buf.data() + at[i - bi]; z.avail_out = (unsigned)blks[i].out_len;
                    if (inflate(&z, Z_FINISH) != Z_STREAM_END || z.avail_out != 0) bad = 1;  // (less data than ISIZE promised would leave stale bytes in the window)
                    inflateEnd(&z);
                }
            };
            const size_t nt = std::min<size_t>(std::max<size_t>(1, (bj - bi) / 16), std::max(1u, std::min(32u, bsx_usable_cpus())));
            std::vector<std::thread> th;
            for (size_t t = 1; t < nt; t++) th.emplace_back(work);
            work();
            for (std::thread &x : th) x.join();
            if (bad) return 1;
        }
        const unsigned char *b = buf.data(), *e = b + carry + out, *q = b;
        bi = bj;
        if (!header_done) {  // magic, text, reference names; all of it must be inside the buffer before it is read
            if (e - b >= 4 && memcmp(b, "BAM\1", 4) != 0) return 1;
            if (e - b >= 8 && rd32(b + 4) < 0) return 1;
            bool complete = e - b >= 12 && (size_t)(e - b) >= (size_t)12 + (size_t)rd32(b + 4);
            if (complete) {
                q = b + 8 + rd32(b + 4);
                n_ref = rd32(q); q += 4;
                if (n_ref < 0) return 1;
                ref_id.clear();
                for (int32_t r = 0; r < n_ref && complete; r++) {
                    if ((size_t)(e - q) < 4) { complete = false; break; }
                    const int32_t ln = rd32(q);
                    if (ln < 1) return 1;
                    if ((size_t)(e - q) < (size_t)4 + (size_t)ln + 4) { complete = false; break; }
                    auto it = cid.find(std::string((const char *)q + 4, strnlen((const char *)q + 4, (size_t)ln)));
                    ref_id.push_back(it == cid.end() ? -1 : (int64_t)it->second);
                    q += 4 + ln + 4;
                }
            }
            if (!complete) { carry += out; continue; }  // header longer than the window so far: read on
            header_done = true;
        }
        ParsedChunk o;
        while ((size_t)(e - q) >= 4) {
            const int32_t bs = rd32(q);
            if (bs < 32) return 1;
            if ((size_t)(e - q) < (size_t)4 + (size_t)bs) break;  // the rest of this record is in the next window
            const unsigned char *r = q + 4;
            q += 4 + (size_t)bs;
            o.lines++;
            const int32_t tid = rd32(r), pos = rd32(r + 4), l_seq = rd32(r + 16), npos = rd32(r + 24), tlen = rd32(r + 28);
            const unsigned l_name = r[8], n_cigar = r[12] | (r[13] << 8), flag = r[14] | (r[15] << 8);
            if ((flag & 0x4) || (unique && (flag & 0x100)) || (pair && !(flag & 0x2))) continue;
            if (tid < 0 || tid >= n_ref || ref_id[(size_t)tid] < 0) continue;
            // name, CIGAR, packed bases and qualities must fit into the record before a pointer to any of them is formed
            if (l_seq < 0 || (size_t)32 + l_name + (size_t)4 * n_cigar + ((size_t)l_seq + 1) / 2 + (size_t)l_seq > (size_t)bs) return 1;
            const unsigned char *sq = r + 32 + l_name + 4 * n_cigar, *ql = sq + ((size_t)l_seq + 1) / 2, *aux = ql + l_seq;
            int st = -1;
            while ((size_t)(r + bs - aux) >= 3) {  // optional fields: find ZS:Z
                const unsigned char t0 = aux[0], t1 = aux[1], ty = aux[2];
                aux += 3;
                const size_t left = (size_t)(r + bs - aux);
                size_t step;
                if (ty == 'Z' || ty == 'H') {
                    const size_t n = strnlen((const char *)aux, left);
                    if (t0 == 'Z' && t1 == 'S' && ty == 'Z' && n >= 2) { st = (aux[0] == '-' ? 1 : 0) | (aux[1] == '-' ? 2 : 0); break; }
                    step = n + 1;
                } else if (ty == 'A' || ty == 'c' || ty == 'C') step = 1;
                else if (ty == 's' || ty == 'S') step = 2;
                else if (ty == 'i' || ty == 'I' || ty == 'f') step = 4;
                else if (ty == 'B') {
                    if (left < 5) break;
                    const unsigned char sub = aux[0];
                    const int32_t cnt = rd32(aux + 1);
                    if (cnt < 0) return 1;  // (a negative count would walk backwards through the record)
                    step = 5 + (size_t)cnt * ((sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4);
                } else break;
                if (step > left) break;  // a field that runs past the record: nothing behind it
                aux += step;
            }
            if (st < 0) { bad_records = 2; continue; }
            o.chr.push_back((uint32_t)ref_id[(size_t)tid]); o.pos.push_back(pos); o.strand.push_back((uint8_t)st); o.insert.push_back(tlen);
            o.cut.push_back(tlen > 0 ? (int64_t)npos : -1);
            for (int32_t i = 0; i < l_seq; i++) o.seq.push_back(nt16[(sq[i >> 1] >> ((~i & 1) << 2)) & 0xf]);
            o.off.push_back(o.seq.size());
        }
        lines += o.lines;
        if (!o.chr.empty()) { const int rc = flush(o); if (rc) return rc; }
        carry = (size_t)(e - q);
        if (carry) memmove(buf.data(), q, carry);
    }
    if (!header_done || carry) return 1;  // no header, or a record cut off by the end of the file
    return 0;
}

// methratio.py:67-77 on a memory map: a record starts at a line whose first character is '>', its name is the first
// token of line[1:-1], its sequence the concatenation of the stripped lines, upper-cased; `chroms_csv` is the -c filter.
// Returns 0, or 1 when no record is selected.
inline int parse_fasta(const char *base, size_t len, const char *chroms_csv, std::vector<std::string> &names, std::vector<std::vector<char>> &seqs)
{
    std::vector<std::string> want;
    if (chroms_csv && *chroms_csv) { std::string t(chroms_csv); size_t a = 0; for (;;) { const size_t c = t.find(',', a); want.push_back(t.substr(a, c == std::string::npos ? c : c - a)); if (c == std::string::npos) break; a = c + 1; } }
    auto wanted = [&](const std::string &n) { if (want.empty()) return true; for (const std::string &w : want) if (w == n) return true; return false; };
    struct Rec { std::string name; size_t b, e; };
    std::vector<Rec> recs;
    {   // header lines
        size_t p = 0;
        std::string cur; bool have = false; size_t sb = 0;
        while (p < len) {
            const char *nl = (const char *)memchr(base + p, '\n', len - p);
            const size_t le = nl ? (size_t)(nl - base) + 1 : len;  // line including its newline
            if (base[p] == '>') {
                if (have && wanted(cur)) recs.push_back(Rec{cur, sb, p});
                // name = line[1:-1].split()[0]
                size_t a = p + 1, z = le > p + 1 ? le - 1 : p + 1;
                while (a < z && (base[a] == ' ' || (base[a] >= '\t' && base[a] <= '\r'))) a++;
                size_t q = a;
                while (q < z && !(base[q] == ' ' || (base[q] >= '\t' && base[q] <= '\r'))) q++;
                cur.assign(base + a, q - a); have = true; sb = le;
                p = le;
                continue;
            }
            // jump to the next header line
            const char *g = p < len ? (const char *)memmem(base + p, len - p, "\n>", 2) : nullptr;
            p = g ? (size_t)(g - base) + 1 : len;
        }
        if (have && wanted(cur)) recs.push_back(Rec{cur, sb, len});
    }
    // (a name given twice keeps its last record, as the reference's dict does)
    for (size_t i = 0; i < recs.size(); i++) for (size_t j = i + 1; j < recs.size(); j++) if (recs[i].name == recs[j].name) { recs.erase(recs.begin() + (long)i); i--; break; }
    if (recs.empty()) return 1;
    seqs.assign(recs.size(), std::vector<char>());
    {
        std::atomic<size_t> next(0);
        auto work = [&] {
            for (size_t i; (i = next.fetch_add(1)) < recs.size();) {
                std::vector<char> &o = seqs[i];
                o.reserve(recs[i].e - recs[i].b);
                size_t p = recs[i].b;
                while (p < recs[i].e) {
                    const char *nl = (const char *)memchr(base + p, '\n', recs[i].e - p);
                    size_t a = p, z = nl ? (size_t)(nl - base) : recs[i].e;
                    p = nl ? (size_t)(nl - base) + 1 : recs[i].e;
                    while (a < z && (base[a] == ' ' || (base[a] >= '\t' && base[a] <= '\r'))) a++;     // line.strip()
                    while (z > a && (base[z - 1] == ' ' || (base[z - 1] >= '\t' && base[z - 1] <= '\r'))) z--;
                    const size_t o0 = o.size();
                    o.insert(o.end(), base + a, base + z);
                    for (size_t k = o0; k < o.size(); k++) if (o[k] >= 'a' && o[k] <= 'z') o[k] = (char)(o[k] - 32);
                }
            }
        };
        const size_t nt = std::min<size_t>(recs.size(), std::max(1u, std::min(32u, bsx_usable_cpus())));
        std::vector<std::thread> th;
        for (size_t t = 1; t < nt; t++) th.emplace_back(work);
        work();
        for (std::thread &x : th) x.join();
    }
    names.clear();
    for (const Rec &r : recs) names.push_back(r.name);
    return 0;
}

// The intervals of a BED file (bsx_meth_write_regions), in the file's order.  A line ends at '\n'; one '\r' in front of it is dropped.  Skipped: an empty
// line, a line of blanks, a line that starts with '#', "track" or "browser".  Columns are separated by runs of tabs and spaces: name, start (0-based), end
// (exclusive), an optional label ("." when absent); further columns are ignored.  start and end are 1 to 18 decimal digits and nothing else.  A record
// whose name `cid` does not hold is dropped and counted (after its numbers have been checked).  end is clipped to the sequence's length, then start to end.
struct BedRecords {
    std::vector<uint32_t> chr, start, end;
    std::vector<std::string> label;
    u64 dropped = 0;
};

inline bool bed_number(const char *b, size_t n, u64 &v)
{
    if (n < 1 || n > 18) return false;
    v = 0;
    for (size_t i = 0; i < n; i++) { if (b[i] < '0' || b[i] > '9') return false; v = v * 10 + (u64)(b[i] - '0'); }
    return true;
}

// Returns 0, or the 1-based number of the first line with fewer than three columns, a start or end that is no number, or start > end (`o` is then void).
// chr_len[id]: the sequences' lengths (below 2^32).
inline u64 parse_bed(const char *base, size_t len, const std::unordered_map<std::string, uint32_t> &cid, const std::vector<u64> &chr_len, BedRecords &o)
{
    const char *p = base, *const e = base + len;
    u64 line = 0;
    std::string key;
    while (p < e) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p));
        const char *le = nl ? nl : e;  // line without its newline
        const char *b = p;
        p = nl ? nl + 1 : e;
        line++;
        if (le > b && le[-1] == '\r') le--;
        const size_t n = (size_t)(le - b);
        if (!n || b[0] == '#' || (n >= 5 && !memcmp(b, "track", 5)) || (n >= 7 && !memcmp(b, "browser", 7))) continue;
        const char *tok[4]; size_t tlen[4];
        int nt = 0;
        for (const char *q = b; q < le && nt < 4;) {
            while (q < le && (*q == ' ' || *q == '\t')) q++;
            if (q == le) break;
            tok[nt] = q;
            while (q < le && *q != ' ' && *q != '\t') q++;
            tlen[nt] = (size_t)(q - tok[nt]);
            nt++;
        }
        if (!nt) continue;
        u64 s, t;
        if (nt < 3 || !bed_number(tok[1], tlen[1], s) || !bed_number(tok[2], tlen[2], t) || s > t) return line;
        key.assign(tok[0], tlen[0]);
        const auto it = cid.find(key);
        if (it == cid.end() || it->second >= chr_len.size()) { o.dropped++; continue; }
        const u64 cl = std::min<u64>(chr_len[it->second], 0xffffffffull);
        t = std::min(t, cl); s = std::min(s, t);
        o.chr.push_back(it->second); o.start.push_back((uint32_t)s); o.end.push_back((uint32_t)t);
        o.label.push_back(nt > 3 ? std::string(tok[3], tlen[3]) : std::string("."));
    }
    return 0;
}

}  // namespace bsx_meth_parse
