// Test harness (ours): the formatter of the epiallele file (bsx_meth_epi::header / append_row of bsmap_amd/csrc/bsx_meth_epi.h), built with
// AddressSanitizer + UndefinedBehaviorSanitizer.
//   epi_check < rows
//       stdin: one window per line, "name pos0 pos0 pos0 pos0 n_0 .. n_15" separated by blanks (0-based positions, a sum of counts of at least 1);
//       stdout: the header, then one formatted row per line of input.  Exit status 2 on a line that does not parse.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../bsmap_amd/csrc/bsx_meth_epi.h"

int main()
{
    std::string out = bsx_meth_epi::header();
    char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        char name[256];
        uint32_t pos[4], counts[16];
        int used = 0;
        if (sscanf(line, "%255s%n", name, &used) != 1) return 2;
        const char *p = line + used;
        uint64_t sum = 0;
        for (int k = 0; k < 20; k++) {
            uint32_t v;
            int n = 0;
            if (sscanf(p, "%" SCNu32 "%n", &v, &n) != 1) return 2;
            p += n;
            if (k < 4) pos[k] = v; else { counts[k - 4] = v; sum += v; }
        }
        if (!sum) return 2;
        bsx_meth_epi::append_row(out, name, pos, counts);
    }
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
