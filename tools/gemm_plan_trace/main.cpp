// Dispatch-trace driver: reads one descriptor per line (51 integers, the order of tests/gemm_plan_corpus.py FIELDS), calls insv2v_gemm
// and the two query functions, prints the return codes.  Linked with the four GEMM objects compiled with -include stub.h.
#include "insv2v_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
bool insv2v_one_device_check() { return true; }
int insv2v_num_cus() { const char* e = getenv("HARNESS_CUS"); return e ? atoi(e) : 256; }   // (the parent has its own copies, stubbed)
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    if (getenv("HARNESS_WINDOW")) insv2v_set_operand_window(atoll(getenv("HARNESS_WINDOW")));
    long long v[51];
    for (long n = 0;; ++n) {
        for (int i = 0; i < 51; ++i)
            if (fscanf(f, "%lld", &v[i]) != 1) return i == 0 ? 0 : 3;
        insv2v_gemm_desc d;
        memset(&d, 0, sizeof d);
        int i = 0;
        auto P = [&] { return (void*)(uintptr_t)v[i++]; };
        d.a = P(); d.a2 = P(); d.w = P(); d.c = P(); d.bias = (const float*)P(); d.row_bias = (const float*)P(); d.residual = P();
        d.row_stats = (const float*)P(); d.col_sum = (const float*)P();
        d.lda = v[i++]; d.lda2 = v[i++]; d.ldw = v[i++]; d.ldc = v[i++]; d.ldr = v[i++]; d.ld_rb = v[i++];
        d.a_bs = v[i++]; d.w_bs = v[i++]; d.c_bs = v[i++]; d.r_bs = v[i++];
        d.workspace = P(); d.workspace_bytes = v[i++];
        int32_t* q[] = {&d.M, &d.N, &d.K, &d.k_split, &d.rows_per_group, &d.rb_mod, &d.act, &d.c_fp32, &d.mode, &d.NB, &d.IH, &d.IW, &d.OH, &d.OW, &d.Cin,
                        &d.stride, &d.pad_t, &d.pad_l, &d.upsample, &d.batch, &d.tile, &d.split_k};
        for (int32_t* p : q) *p = (int32_t)v[i++];
        d.gn_ab = (const float*)P(); d.gn_images_per_sample = (int32_t)v[i++]; d.gn_silu = (int32_t)v[i++];
        d.stats_out = (float*)P(); d.stats_scratch = (float*)P(); d.stats_parts = (int32_t)v[i++];
        d.w_group_stride = v[i++]; d.w_group_rows = (int32_t)v[i++];
        d.ln_eps = 1e-5f;
        printf("#%ld\n", n);
        const int rc = insv2v_gemm(&d, 0);
        printf("rc %d parts %d fuses %d\n", rc, insv2v_gemm_stats_parts(&d), insv2v_conv3x3_fuses_groupnorm(&d));
    }
}
