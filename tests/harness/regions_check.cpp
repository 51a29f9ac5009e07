// Test harness (ours): the BED parser of the methylation-ratio tool (bsx_meth_parse::parse_bed of bsmap_amd/csrc/bsx_meth_parse.h) on one file, built
// with AddressSanitizer + UndefinedBehaviorSanitizer.  The file is read into a heap block of exactly its size, so that a read one byte past it is reported.
//   regions_check bed <file> <names,comma,separated> <lengths,comma,separated>
//       one line "chr<TAB>start<TAB>end<TAB>label" per record kept (chr as its id), then "records N dropped M" — or "error line N"
//   regions_check prefixes <file> <names> <lengths>
//       the file cut off after every byte count 0..size, each prefix parsed from a heap block of its own size: "<bytes> records N dropped M" or
//       "<bytes> error line N"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../bsmap_amd/csrc/bsx_meth_parse.h"

namespace P = bsx_meth_parse;

static std::vector<std::string> split(const char *txt)
{
    std::vector<std::string> out;
    std::string t(txt);
    size_t a = 0;
    for (;;) { const size_t c = t.find(',', a); out.push_back(t.substr(a, c == std::string::npos ? c : c - a)); if (c == std::string::npos) break; a = c + 1; }
    return out;
}

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const size_t len = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    char *base = new char[len ? len : 1];
    if (len && fread(base, 1, len, f) != len) return 2;
    fclose(f);
    std::unordered_map<std::string, uint32_t> cid;
    std::vector<P::u64> lens;
    {
        const std::vector<std::string> names = split(argv[3]), ls = split(argv[4]);
        if (names.size() != ls.size()) return 2;
        for (size_t i = 0; i < names.size(); i++) { cid.emplace(names[i], (uint32_t)i); lens.push_back(strtoull(ls[i].c_str(), nullptr, 10)); }
    }
    int rc = 0;
    try {
        if (!strcmp(argv[1], "bed")) {
            P::BedRecords o;
            const P::u64 bad = P::parse_bed(base, len, cid, lens, o);
            if (bad) printf("error line %llu\n", bad);
            else {
                for (size_t i = 0; i < o.chr.size(); i++) printf("%u\t%u\t%u\t%s\n", o.chr[i], o.start[i], o.end[i], o.label[i].c_str());
                printf("records %zu dropped %llu\n", o.chr.size(), o.dropped);
            }
        } else if (!strcmp(argv[1], "prefixes")) {
            for (size_t n = 0; n <= len; n++) {
                char *part = new char[n ? n : 1];
                memcpy(part, base, n);
                P::BedRecords o;
                const P::u64 bad = P::parse_bed(part, n, cid, lens, o);
                if (bad) printf("%zu error line %llu\n", n, bad);
                else printf("%zu records %zu dropped %llu\n", n, o.chr.size(), o.dropped);
                delete[] part;
            }
        } else rc = 2;
    } catch (const std::bad_alloc &) {
        printf("error nomem\n");
    }
    delete[] base;
    return rc;
}
