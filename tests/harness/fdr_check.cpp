// Test harness (ours): the q-value and DMR formatters, the delta rule's host form and the run filter of bsmap_amd/csrc/bsx_meth_diff.h on the host, built
// with AddressSanitizer + UndefinedBehaviorSanitizer.
//   fdr_check < lines
//       stdin, one request per line, fields separated by blanks:
//           hdr                                              -> the position, region and DMR headers of the q-value files
//           posq name pos0 cls mA dA mB dB p q               -> the row of the position file with q
//           regq name start end label N MA DA MB DB p q      -> the row of the region file with q
//           dmr name start end n_sig N MA DA MB DB p         -> the row of the DMR file
//           keep permille mA dA mB dB                        -> "<delta_keeps as 0 / 1> <delta_sign>"
//           runs min_sites n (chr start end n_sig) x n       -> the runs keep_runs leaves, one per line
//       p and q are read by strtod ("%la": hexadecimal floats and nan are accepted).  Exit status 2 on a line that does not parse.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../bsmap_amd/csrc/bsx_meth_diff.h"

int main()
{
    std::string out;
    static char line[1 << 16];
    char num[128];
    while (fgets(line, sizeof(line), stdin)) {
        char kind[8], name[256], label[256];
        uint64_t v[5];
        uint32_t a, b, c;
        double p, q;
        if (sscanf(line, "%7s", kind) != 1) return 2;
        if (!strcmp(kind, "hdr")) {
            out += bsx_meth_diff::POS_FDR_HEADER; out += bsx_meth_diff::REGION_FDR_HEADER; out += bsx_meth_diff::DMR_HEADER;
        } else if (!strcmp(kind, "posq")) {
            if (sscanf(line, "%*s %255s %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %la %la", name, &a, &b, &v[0], &v[1], &v[2], &v[3], &p, &q) != 9)
                return 2;
            const uint32_t counts[4] = {(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3]};
            bsx_meth_diff::append_pos_row(out, name, a, (uint8_t)b, counts, p);
            bsx_meth_diff::append_q(out, q);
        } else if (!strcmp(kind, "regq")) {
            if (sscanf(line, "%*s %255s %" SCNu32 " %" SCNu32 " %255s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %la %la", name, &a, &b, label, &v[0], &v[1],
                       &v[2], &v[3], &v[4], &p, &q) != 11)
                return 2;
            const std::string l(label);
            bsx_meth_diff::append_interval_row(out, name, a, b, &l, v, p);
            bsx_meth_diff::append_q(out, q);
        } else if (!strcmp(kind, "dmr")) {
            if (sscanf(line, "%*s %255s %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %la", name, &a, &b, &c, &v[0], &v[1], &v[2],
                       &v[3], &v[4], &p) != 10)
                return 2;
            bsx_meth_diff::append_dmr_row(out, name, a, b, c, v, p);
        } else if (!strcmp(kind, "keep")) {
            if (sscanf(line, "%*s %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &a, &v[0], &v[1], &v[2], &v[3]) != 5) return 2;
            out.append(num, (size_t)snprintf(num, sizeof(num), "%d %d\n", (int)bsx_meth_diff::delta_keeps((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], a),
                                             bsx_meth_diff::delta_sign((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3])));
        } else if (!strcmp(kind, "runs")) {
            char *at = line + 4;
            const uint32_t min_sites = (uint32_t)strtoul(at, &at, 10);
            const size_t n = strtoul(at, &at, 10);
            std::vector<uint32_t> runs(n * 4);
            for (uint32_t &x : runs) {
                char *end = nullptr;
                x = (uint32_t)strtoul(at, &end, 10);
                if (end == at) return 2;
                at = end;
            }
            const size_t kept = bsx_meth_diff::keep_runs(runs.data(), n, min_sites);
            for (size_t i = 0; i < kept; i++)
                out.append(num, (size_t)snprintf(num, sizeof(num), "%u %u %u %u\n", runs[i * 4], runs[i * 4 + 1], runs[i * 4 + 2], runs[i * 4 + 3]));
            out += "-\n";
        } else
            return 2;
    }
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}
