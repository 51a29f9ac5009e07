// Test harness (ours): the row formatters of bsmap_amd/csrc/bsx_meth_text.h (the table with 9 and 12 columns, the region file, the wiggle track, the PDR
// file), built with AddressSanitizer + UndefinedBehaviorSanitizer.
//   meth_text_check < rows
//       stdin: one row per line, a kind and its fields separated by blanks (all numbers unsigned decimal):
//           table9  name pos0 depth meth ctx                  ctx: the packed context of k_meth_emit
//           table12 name pos0 depth meth ctx rev_g rev_ga
//           region  name start end label N M D E MC
//           wig     j bin N M D E MC
//           pdr     name pos0 letter reads discordant         letter: the reference letter, C or G
//       stdout: one formatted line per line of input (none for a wig line without a ratio).  Exit status 2 on a line that does not parse.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../bsmap_amd/csrc/bsx_meth_text.h"

int main()
{
    std::string out;
    static char line[1 << 16], name[1 << 15], label[1 << 15];
    while (fgets(line, sizeof(line), stdin)) {
        char kind[16];
        int used = 0;
        if (sscanf(line, "%15s%n", kind, &used) != 1) return 2;
        const char *p = line + used;
        if (!strcmp(kind, "table9") || !strcmp(kind, "table12")) {
            const bool snp = !strcmp(kind, "table12");
            uint32_t pos0, depth, meth, g = 0, ga = 0;
            uint64_t ctx;
            if (sscanf(p, "%32767s %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64 "%n", name, &pos0, &depth, &meth, &ctx, &used) != 5) return 2;
            if (snp && sscanf(p + used, "%" SCNu32 " %" SCNu32, &g, &ga) != 2) return 2;
            bsx_meth_text::append_table_row(out, name, pos0, depth, meth, ctx, snp, g, ga);
        } else if (!strcmp(kind, "region")) {
            uint32_t start, end;
            uint64_t s[5];
            if (sscanf(p, "%32767s %" SCNu32 " %" SCNu32 " %32767s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, name, &start, &end, label, &s[0], &s[1], &s[2], &s[3],
                       &s[4]) != 9)
                return 2;
            bsx_meth_text::append_region_row(out, name, start, end, label, s);
        } else if (!strcmp(kind, "wig")) {
            uint64_t j, s[5];
            uint32_t bin;
            if (sscanf(p, "%" SCNu64 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &j, &bin, &s[0], &s[1], &s[2], &s[3], &s[4]) != 7) return 2;
            bsx_meth_text::append_wig_line(out, j, bin, s);
        } else if (!strcmp(kind, "pdr")) {
            uint32_t pos0, reads, disc;
            char letter;
            if (sscanf(p, "%32767s %" SCNu32 " %c %" SCNu32 " %" SCNu32, name, &pos0, &letter, &reads, &disc) != 5 || !reads) return 2;
            bsx_meth_text::append_pdr_row(out, name, pos0, (uint8_t)letter, reads, disc);
        } else
            return 2;
    }
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
