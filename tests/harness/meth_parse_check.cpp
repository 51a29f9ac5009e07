// Test harness (ours): the methylation-ratio tool's file parsers (bsmap_amd/csrc/bsx_meth_parse.h) on one file, built with
// AddressSanitizer + UndefinedBehaviorSanitizer.  The file is read into a heap block of exactly its size, so that a read one
// byte past it is reported.
//   meth_parse_check aln <file> <0 BSP | 1 SAM | 2 BAM> <names,comma,separated> <unique> <pair> <bam window> <text piece>
//       one line "chr<TAB>pos<TAB>strand<TAB>insert<TAB>cut<TAB>seq" per alignment that passes the filters (pos 0-based, cut = PNEXT-1 or -1),
//       "-- flush N" after every hand-over of N alignments, then "lines N" — or "error N" (1 malformed file, 2 no strand information)
//   meth_parse_check prefixes <file> 2 <names> <unique> <pair> <bam window> <dense> <stride>
//       the BAM file cut off after every byte count below <dense>, then after every <stride>-th: one line "<bytes> lines N alignments M"
//       or "<bytes> error N" per prefix, each prefix parsed from a heap block of its own size
//   meth_parse_check fasta <file> <names,comma,separated or ->
//       one line "name<TAB>letters" per selected record, or "error 1"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../bsmap_amd/csrc/bsx_meth_parse.h"

namespace P = bsx_meth_parse;

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const size_t len = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    char *base = new char[len ? len : 1];
    if (len && fread(base, 1, len, f) != len) return 2;
    fclose(f);
    int rc = 0;
    try {
        if (!strcmp(argv[1], "fasta")) {
            std::vector<std::string> names;
            std::vector<std::vector<char>> seqs;
            const int e = len ? P::parse_fasta(base, len, strcmp(argv[3], "-") ? argv[3] : nullptr, names, seqs) : 1;
            if (e) printf("error %d\n", e);
            else for (size_t i = 0; i < names.size(); i++) { printf("%s\t", names[i].c_str()); fwrite(seqs[i].data(), 1, seqs[i].size(), stdout); putchar('\n'); }
        } else if (!strcmp(argv[1], "aln") && argc >= 9) {
            const int sam = atoi(argv[3]), unique = atoi(argv[5]), pair = atoi(argv[6]);
            const size_t window = (size_t)atoll(argv[7]), piece = (size_t)atoll(argv[8]);
            std::vector<std::string> names;
            std::unordered_map<std::string, uint32_t> cid;
            {
                std::string t(argv[4]);
                size_t a = 0;
                for (;;) { const size_t c = t.find(',', a); names.push_back(t.substr(a, c == std::string::npos ? c : c - a)); if (c == std::string::npos) break; a = c + 1; }
                for (size_t i = 0; i < names.size(); i++) cid.emplace(names[i], (uint32_t)i);
            }
            static const char *const strands[4] = {"++", "-+", "+-", "--"};
            auto flush = [&](P::ParsedChunk &o) {
                for (size_t i = 0; i < o.chr.size(); i++) {
                    printf("%s\t%lld\t%s\t%d\t%lld\t", names[o.chr[i]].c_str(), (long long)o.pos[i], strands[o.strand[i] & 3], o.insert[i], (long long)o.cut[i]);
                    fwrite(o.seq.data() + o.off[i], 1, (size_t)(o.off[i + 1] - o.off[i]), stdout);
                    putchar('\n');
                }
                printf("-- flush %zu\n", o.chr.size());
                return 0;
            };
            P::u64 lines = 0;
            int bad = 0, e;
            if (sam == 2) { e = P::stream_bam(base, len, cid, unique, pair, window, lines, bad, flush); if (!e && bad == 2) e = 2; }
            else e = P::stream_text(base, len, sam, cid, unique, pair, piece, lines, flush);
            if (e) printf("error %d\n", e);
            else printf("lines %llu\n", lines);
        } else if (!strcmp(argv[1], "prefixes") && argc >= 10) {
            const int unique = atoi(argv[5]), pair = atoi(argv[6]);
            const size_t window = (size_t)atoll(argv[7]), dense = (size_t)atoll(argv[8]), stride = (size_t)std::max(1ll, atoll(argv[9]));
            std::unordered_map<std::string, uint32_t> cid;
            {
                std::string t(argv[4]);
                size_t a = 0;
                uint32_t k = 0;
                for (;;) { const size_t c = t.find(',', a); cid.emplace(t.substr(a, c == std::string::npos ? c : c - a), k++); if (c == std::string::npos) break; a = c + 1; }
            }
            for (size_t n = 0; n <= len; n += (n < dense ? 1 : stride)) {
                char *part = new char[n ? n : 1];
                memcpy(part, base, n);
                P::u64 lines = 0, alns = 0;
                int bad = 0;
                const int e = P::stream_bam(part, n, cid, unique, pair, window, lines, bad, [&](P::ParsedChunk &o) { alns += o.chr.size(); return 0; });
                if (e) printf("%zu error %d\n", n, e);
                else printf("%zu lines %llu alignments %llu\n", n, lines, alns);
                delete[] part;
            }
        } else rc = 2;
    } catch (const std::bad_alloc &) {
        printf("error nomem\n");
    }
    delete[] base;
    return rc;
}
