// ctc_abi_check.cpp — the host-side argument checks of the CTC entry points (include/rnnt_engine.h rnnt_engine_ctc_*) as a
// stand-alone program: the size query over U, and every refusing path (nothing is launched, no GPU is needed).  Meant for a
// host sanitizer, which checks only code linked into a program of its own:
//   cd rnnt_amd/csrc && make && hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -Xarch_host -fsanitize=address -c engine.hip -o /tmp/engine_asan.o
//   clang++ -O1 -g -std=c++17 -fsanitize=address -c ../../tools/ctc_abi_check.cpp -o /tmp/ctc_abi_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address /tmp/ctc_abi_check.o /tmp/engine_asan.o $(ls *.o | grep -v '^engine.o$') -o ../../tools/ctc_abi_check
//   ../../tools/ctc_abi_check        # prints "ok (0 failures)"
#include <cstdio>
#include <cstring>
#include "../include/rnnt_engine.h"
static int fails = 0;
#define EXPECT(call, code, word) do { int rc = (call); const char *m = rnnt_engine_last_error(); \
    if (rc != (code) || (word[0] && !strstr(m, word))) { printf("FAIL %s -> %d '%s'\n", #call, rc, m); ++fails; } } while (0)
int main()
{
    size_t n = 0, prev = 0;
    void *P = (void *)4096;
    for (int U = 0; U <= 1023; U += 93) { EXPECT(rnnt_engine_ctc_workspace_bytes(3, 70, U, 32, &n), 0, ""); if (n <= prev || n % 256) { printf("FAIL size U=%d\n", U); ++fails; } prev = n; }
    EXPECT(rnnt_engine_ctc_workspace_bytes(2, 50, 1024, 32, &n), RNNT_ERR_UNSUPPORTED, "1023");
    EXPECT(rnnt_engine_ctc_workspace_bytes(2, 50, 10, 6, &n), RNNT_ERR_UNSUPPORTED, "multiple of 4");
    EXPECT(rnnt_engine_ctc_workspace_bytes(2, 50, 10, 32, nullptr), RNNT_ERR_INVALID_ARG, "null");
    EXPECT(rnnt_engine_ctc_workspace_bytes(0, 50, 10, 32, &n), RNNT_ERR_INVALID_ARG, "non-positive");
    const int32_t *I = (const int32_t *)P; float *F = (float *)P;
    EXPECT(rnnt_engine_ctc_loss_fwd_bwd(P, I, I, I, 2, 50, 1024, 32, 31, nullptr, F, F, P, (size_t)1 << 40, nullptr), RNNT_ERR_UNSUPPORTED, "U=1024");
    EXPECT(rnnt_engine_ctc_loss_fwd_bwd(P, I, I, I, 2, 50, 10, 6, 5, nullptr, F, F, P, (size_t)1 << 40, nullptr), RNNT_ERR_UNSUPPORTED, "V=6");
    EXPECT(rnnt_engine_ctc_loss_fwd_bwd(P, I, I, I, 2, 50, 10, 32, 32, nullptr, F, F, P, (size_t)1 << 40, nullptr), RNNT_ERR_INVALID_ARG, "blank=32");
    EXPECT(rnnt_engine_ctc_loss_fwd_bwd(nullptr, I, I, I, 2, 50, 10, 32, 31, nullptr, F, F, P, (size_t)1 << 40, nullptr), RNNT_ERR_INVALID_ARG, "null");
    EXPECT(rnnt_engine_ctc_loss_fwd_bwd(P, I, I, I, 2, 50, 10, 32, 31, nullptr, nullptr, F, P, (size_t)1 << 40, nullptr), RNNT_ERR_INVALID_ARG, "null");
    EXPECT(rnnt_engine_ctc_loss_fwd_bwd(P, I, I, I, 2, 50, 10, 32, 31, nullptr, F, F, nullptr, (size_t)1 << 40, nullptr), RNNT_ERR_INVALID_ARG, "null");
    rnnt_engine_ctc_workspace_bytes(2, 50, 10, 32, &n);
    EXPECT(rnnt_engine_ctc_loss_fwd_bwd(P, I, I, I, 2, 50, 10, 32, 31, nullptr, F, F, P, n - 1, nullptr), RNNT_ERR_WORKSPACE, "workspace");
    EXPECT(rnnt_engine_ctc_loss_fwd_bwd((void *)4100, I, I, I, 2, 50, 10, 32, 31, nullptr, F, F, P, n, nullptr), RNNT_ERR_INVALID_ARG, "aligned");
    int32_t *O = (int32_t *)P;
    EXPECT(rnnt_engine_ctc_greedy_decode(P, I, 2, 50, 6, 5, O, O, nullptr), RNNT_ERR_UNSUPPORTED, "multiple of 4");
    EXPECT(rnnt_engine_ctc_greedy_decode(P, I, 2, 50, 32, 32, O, O, nullptr), RNNT_ERR_INVALID_ARG, "blank=32");
    EXPECT(rnnt_engine_ctc_greedy_decode(nullptr, I, 2, 50, 32, 31, O, O, nullptr), RNNT_ERR_INVALID_ARG, "null");
    EXPECT(rnnt_engine_ctc_greedy_decode(P, I, 2, 50, 32, 31, O, nullptr, nullptr), RNNT_ERR_INVALID_ARG, "null");
    EXPECT(rnnt_engine_ctc_greedy_decode(P, I, 0, 50, 32, 31, O, O, nullptr), RNNT_ERR_INVALID_ARG, "non-positive");
    printf("%s (%d failures)\n", fails ? "FAILED" : "ok", fails);
    return fails != 0;
}
