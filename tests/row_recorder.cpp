// Host-only recorder of the row-kernel dispatch (tests/row_witness.py builds and runs it): the sibling of tests/dispatch_recorder.cpp.
// Links csrc/rowops.o and inorm.o WITHOUT the HIP runtime, against the stubs of tests/hip_stubs.h, reads one call per line from
// standard input, as plain numbers (a flag is 0 | 1, one per optional pointer or switch of the entry point),
//   LF <dtype rows C ld> <gamma/beta residual gelu>                        gwd_layernorm_forward          (ld 0 = C)
//   LB <dtype rows C ld> <gamma/beta gelu gskip elu_input dgamma>          gwd_layernorm_backward         (elu_input: GWD_LN_ELU_INPUT)
//   SF <dtype rows L>                                                      gwd_softmax_forward
//   SB <dtype rows L>                                                      gwd_softmax_backward
//   SM <dtype rows L> <mask rows_per_mask scale>                           gwd_softmax_masked_forward     (scale: 0 = 1.0 | 1 = 0.3)
//   SS <dtype rows L> <scale>                                              gwd_softmax_scaled_backward
//   AB <dtype rows C> <act act_scale per_channel_scale>                    gwd_act_backward               (act_scale: 0 = 1.0 | 1 = 0.7)
//   CS <dtype rows C>                                                      gwd_colsum
//   CB <dtype n> <rows C> ... n times                                      gwd_colsum_batch
//   AC <dtype rows C> <act act_scale mult>                                 gwd_act_backward_colsum
//   IF <dtype B L C S>                                                     gwd_inorm_gelu_forward
//   IB <dtype B L C S>                                                     gwd_inorm_gelu_backward
// and prints per call   <the line> rc=<return code> { | <mangled kernel> <grid> <block> <dynamic LDS> }.
// A malformed line ends the run with status 2.  The output depends on the host logic of the two objects only.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gwdepth.h"
#include "hip_stubs.h"

namespace {
void *fake(int i) { return (void *)(uintptr_t)(0x100000 + 0x1000 * i); }
float *ffake(int i) { return (float *)fake(i); }

int run(const char *op, const std::vector<long long> &v) {
    const size_t n = v.size();
    auto flag = [&](size_t i, int k) -> void * { return v[i] ? fake(k) : nullptr; };
    const int dtype = n ? (int)v[0] : 0;
    if (!strcmp(op, "LF") && n == 7)
        return gwd_layernorm_forward(fake(0), (float *)flag(4, 1), (float *)flag(4, 2), flag(5, 3), fake(4), ffake(5), ffake(6), v[1], (int)v[2], (int)v[3], (int)v[6], dtype, nullptr);
    if (!strcmp(op, "LB") && n == 9)
        return gwd_layernorm_backward(fake(0), fake(1), (float *)flag(4, 2), (float *)flag(4, 3), ffake(4), ffake(5), fake(6), (float *)flag(8, 7), (float *)flag(8, 8), v[1], (int)v[2],
                                      (int)v[3], (v[5] ? 1 : 0) | (v[7] ? GWD_LN_ELU_INPUT : 0), flag(6, 9), dtype, nullptr);
    if (!strcmp(op, "SF") && n == 3) return gwd_softmax_forward(fake(0), fake(1), v[1], (int)v[2], dtype, nullptr);
    if (!strcmp(op, "SB") && n == 3) return gwd_softmax_backward(fake(0), fake(1), fake(2), v[1], (int)v[2], dtype, nullptr);
    if (!strcmp(op, "SM") && n == 6)
        return gwd_softmax_masked_forward(fake(0), (const uint8_t *)flag(3, 1), fake(2), v[1], (int)v[2], v[3] ? v[4] : 1, v[5] ? 0.3f : 1.0f, dtype, nullptr);
    if (!strcmp(op, "SS") && n == 4) return gwd_softmax_scaled_backward(fake(0), fake(1), fake(2), v[1], (int)v[2], v[3] ? 0.3f : 1.0f, dtype, nullptr);
    if (!strcmp(op, "AB") && n == 6)
        return gwd_act_backward(fake(0), v[3] ? fake(1) : nullptr, fake(2), (float *)flag(5, 3), v[1], (int)v[2], (int)v[3], v[4] ? 0.7f : 1.0f, dtype, nullptr);
    if (!strcmp(op, "CS") && n == 3) return gwd_colsum(fake(0), ffake(1), v[1], (int)v[2], dtype, nullptr);
    if (!strcmp(op, "CB") && n >= 2 && v[1] >= 1 && v[1] <= 64 && n == 2 + 2 * (size_t)v[1]) {
        std::vector<gwd_colsum_job> jobs((size_t)v[1]);
        memset(jobs.data(), 0, jobs.size() * sizeof jobs[0]);
        for (size_t i = 0; i < jobs.size(); ++i) jobs[i].g = fake(2 * (int)i), jobs[i].out = ffake(2 * (int)i + 1), jobs[i].rows = v[2 + 2 * i], jobs[i].C = (int)v[3 + 2 * i];
        return gwd_colsum_batch(jobs.data(), (int)jobs.size(), dtype, nullptr);
    }
    if (!strcmp(op, "AC") && n == 6)
        return gwd_act_backward_colsum(fake(0), v[3] ? fake(1) : nullptr, fake(2), ffake(3), v[1], (int)v[2], (int)v[3], v[4] ? 0.7f : 1.0f, flag(5, 4), dtype, nullptr);
    if (!strcmp(op, "IF") && n == 5) return gwd_inorm_gelu_forward(fake(0), fake(1), fake(2), ffake(3), ffake(4), v[1], v[2], (int)v[3], (int)v[4], 1e-5f, dtype, nullptr);
    if (!strcmp(op, "IB") && n == 5) return gwd_inorm_gelu_backward(fake(0), fake(1), ffake(2), ffake(3), fake(4), v[1], v[2], (int)v[3], (int)v[4], dtype, nullptr);
    return -1000;
}
}  // namespace

int main() {
    static char out_buf[1 << 20];
    setvbuf(stdout, out_buf, _IOFBF, sizeof out_buf);
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        char op[8];
        int used = 0;
        if (sscanf(line, " %7s%n", op, &used) != 1) return 2;
        std::vector<long long> v;
        const char *p = line + used;
        long long x;
        while (sscanf(p, "%lld%n", &x, &used) == 1) v.push_back(x), p += used;
        line[strcspn(line, "\n")] = 0;
        g_line = line;
        const int rc = run(op, v);
        if (rc == -1000) return 2;
        const size_t bar = g_line.find(" | ");
        char buf[24];
        snprintf(buf, sizeof buf, " rc=%d", rc);
        g_line.insert(bar == std::string::npos ? g_line.size() : bar, buf);
        g_line += '\n';
        fwrite(g_line.data(), 1, g_line.size(), stdout);
        g_line.clear();
    }
    return 0;
}
