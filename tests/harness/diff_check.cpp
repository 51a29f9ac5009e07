// Test harness (ours): the Fisher test and the row formatters of bsmap_amd/csrc/bsx_meth_diff.h on the host, built with AddressSanitizer +
// UndefinedBehaviorSanitizer.  The kernel k_meth_fisher compiles the same text of fisher_p for the device.
//   diff_check < lines
//       stdin, one request per line, fields separated by blanks:
//           q mA dA mB dB                              -> p as "%a"
//           pos name pos0 cls mA dA mB dB p            -> the row of the position file (cls: bits 0-1 the context class, bit 2 set over a G)
//           reg name start end label N MA DA MB DB p   -> the row of the region file
//           bin name start end N MA DA MB DB p         -> the row of the bin file
//       p is read by strtod ("%la": hexadecimal floats and nan are accepted).  Exit status 2 on a line that does not parse.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../bsmap_amd/csrc/bsx_meth_diff.h"

int main()
{
    std::string out;
    char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        char kind[8], name[256], label[256];
        uint64_t v[5];
        uint32_t a, b;
        double p;
        if (sscanf(line, "%7s", kind) != 1) return 2;
        if (!strcmp(kind, "q")) {
            if (sscanf(line, "%*s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &v[0], &v[1], &v[2], &v[3]) != 4) return 2;
            char num[64];
            out.append(num, (size_t)snprintf(num, sizeof(num), "%a\n", bsx_meth_diff::fisher_p((double)v[0], (double)v[1], (double)v[2], (double)v[3])));
        } else if (!strcmp(kind, "pos")) {
            if (sscanf(line, "%*s %255s %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %la", name, &a, &b, &v[0], &v[1], &v[2], &v[3], &p) != 8) return 2;
            const uint32_t counts[4] = {(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]};
            bsx_meth_diff::append_pos_row(out, name, a, (uint8_t)b, counts, p);
        } else if (!strcmp(kind, "reg")) {
            if (sscanf(line, "%*s %255s %" SCNu32 " %" SCNu32 " %255s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %la", name, &a, &b, label, &v[0], &v[1], &v[2],
                       &v[3], &v[4], &p) != 10) return 2;
            const std::string l(label);
            bsx_meth_diff::append_interval_row(out, name, a, b, &l, v, p);
        } else if (!strcmp(kind, "bin")) {
            if (sscanf(line, "%*s %255s %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %la", name, &a, &b, &v[0], &v[1], &v[2], &v[3], &v[4],
                       &p) != 9) return 2;
            bsx_meth_diff::append_interval_row(out, name, a, b, nullptr, v, p);
        } else
            return 2;
    }
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
