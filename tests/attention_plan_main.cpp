// Host-only driver of csrc/attention_plan.h for tests/test_attention_plan_host.py: reads lines
//     plan head_dim heads n_seq max_len total_rows ld_qk ld_out out_scales out_aligned16 sw_waves sw_line_stores
// and prints `waves line_stores n_qt workgroups` per line (sw_waves 0 and sw_line_stores -1 are the product library's switches).  A line
// `cls max_len` prints the CLS-only kernel's LDS bytes.
#include <cstdio>
#include <cstring>

#include "../tensor-truth_amd/csrc/attention_plan.h"

int main() {
    char line[256], what[16];
    while (fgets(line, sizeof line, stdin)) {
        if (sscanf(line, "%15s", what) != 1) continue;
        if (!strcmp(what, "cls")) {
            int max_len;
            if (sscanf(line, "%*s %d", &max_len) != 1) return 2;
            printf("%zu\n", attention_cls_lds_bytes(max_len));
            continue;
        }
        if (strcmp(what, "plan")) return 2;
        int head_dim, heads, n_seq, max_len, ld_qk, ld_out, out_scales, aligned;
        long long total_rows;
        AttnSwitches sw;
        if (sscanf(line, "%*s %d %d %d %d %lld %d %d %d %d %d %d", &head_dim, &heads, &n_seq, &max_len, &total_rows, &ld_qk, &ld_out,
                   &out_scales, &aligned, &sw.waves, &sw.line_stores) != 11)
            return 2;
        const AttnPlan p = attention_plan(head_dim, heads, n_seq, max_len, total_rows, ld_qk, ld_out, out_scales != 0, aligned != 0, sw);
        printf("%d %d %d %lld\n", p.waves, p.line_stores ? 1 : 0, p.n_qt, p.workgroups);
    }
    return 0;
}
