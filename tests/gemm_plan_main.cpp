// Host-only driver of csrc/gemm_plan.h for tests/test_gemm_plan_host.py: reads lines
//     form epi M N K lda ldc ldr cu_count        (form: 16 | x3 | fp8 | xc;  epi: the TT_EPI_* number)
// and prints `kernel gridx gridy` per line with the product library's switches (GemmSwitches' defaults).  A line that starts with
// `qkv` instead -- `qkv M N vt_col0 ldc ldvt` -- prints 1 or 0: whether the 16-bit QKV projection runs as two launches.
#include <cstdio>
#include <cstring>

#include "../tensor-truth_amd/csrc/gemm_plan.h"

int main() {
    static const char* const kNames[] = {"Skinny", "Relay", "Staged128", "TwoStage128", "OneTile256", "Persistent256"};
    const GemmSwitches sw;
    char line[256], form[16];
    while (fgets(line, sizeof line, stdin)) {
        int v[8];
        if (sscanf(line, "%15s", form) != 1) continue;
        if (!strcmp(form, "qkv")) {
            if (sscanf(line, "%*s %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4]) != 5) return 2;
            printf("%d\n", gemm_qkv_splits(v[0], v[1], v[2], v[3], v[4], sw) ? 1 : 0);
            continue;
        }
        GemmForm f;
        if (!strcmp(form, "16")) f = GemmForm::Bits16;
        else if (!strcmp(form, "x3")) f = GemmForm::X3;
        else if (!strcmp(form, "fp8")) f = GemmForm::Fp8;
        else if (!strcmp(form, "xc")) f = GemmForm::Xc;
        else return 2;
        // epi M N K lda ldc ldr cu_count (the plan does not depend on lda)
        if (sscanf(line, "%*s %d %d %d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7]) != 8) return 2;
        const GemmPlan p = gemm_plan(f, v[0], v[1], v[2], v[3], v[5], v[6], v[7], sw);
        printf("%s %d %d\n", kNames[(int)p.kernel], p.gx, p.gy);
    }
    return 0;
}
