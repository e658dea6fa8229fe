// Host-only recorder of the convolution dispatch (tests/test_conv_dispatch.py builds and runs it).
// Links csrc/igemm.o, thinconv.o and tileconv.o WITHOUT the HIP runtime: the dozen runtime symbols those objects need are the stubs
// of tests/hip_stubs.h, hipLaunchKernel among them, which prints instead of launching.  Walks a grid of descriptors through gwd_conv_forward,
// gwd_conv_wgrad and gwd_conv_wgrad_batch (and the three weight-copy entry points) and prints one line per call:
//   <call> <descriptor> rc=<return code> { | <mangled kernel> <grid> <block> <dynamic LDS> <int arguments> }
// The output depends on the host logic of the three objects and on the stubbed CU count (256) only.
// With the argument `--stdin` it walks no grid: it reads one call per line from standard input, as plain numbers,
//   F <B Hi Wi Cin Cout k s gather dtype zero_page> <kind 0..11> <ln_C, 0 = Cout> <act_scale: 0 = 1.0 | 1 = 0.7>
//   W <B Hi Wi Cin Cout k s gather dtype zero_page> <scaled 0|1>
//   B <n> <B Hi Wi Cin Cout k s gather dtype zero_page> <scaled 0|1>      n jobs of one layer in one gwd_conv_wgrad_batch call, job i on B + i images
// and prints the same records (tools/make_conv_witnesses.py and tests/test_conv_witnesses.py drive it).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gwdepth.h"
#include "hip_stubs.h"

namespace {
// positions of the scalar int arguments that follow the descriptor (and dw), by kernel
const IntArgs INT_ARGS[] = {{"igemm_dma_kernel", 1, 2},  {"gemm_ksplit_kernel", 1, 1}, {"igemm_wgrad_dma_kernel", 2, 1}, {"igemm_wgrad_kernel", 2, 1},
                            {"wgrad_taps_kernel", 2, 2}, {"tconv_fwd_kernel", 1, 3},   {"tconv_wgrad_kernel", 2, 3},     {"thin_wgrad_kernel", 2, 1}};
}  // namespace

namespace {
// fake device pointers: never dereferenced on the host, 16-byte aligned (tileconv.hip looks at the alignment)
void *fake(int i) { return (void *)(uintptr_t)(0x100000 + 0x1000 * i); }

const char *KINDS[] = {"plain", "bn_relu", "gelu_z", "elu", "mult_res", "mult_relu", "mult_relu_z", "gate_relu", "gate_gelu", "convln", "convln_gelu", "bias_relu_res"};
constexpr int N_KINDS = 12;

void set_epilogue(gwd_conv_desc &d, int kind) {
    switch (kind) {
        case 1: d.scale = (float *)fake(4), d.shift = (float *)fake(5), d.act = GWD_ACT_RELU; break;
        case 2: d.shift = (float *)fake(5), d.act = GWD_ACT_GELU, d.z = fake(3); break;
        case 3: d.shift = (float *)fake(5), d.act = GWD_ACT_ELU; break;
        case 4: d.mult = fake(7), d.residual = fake(6); break;
        case 5: d.mult = fake(7), d.act = GWD_ACT_RELU; break;
        case 6: d.mult = fake(7), d.act = GWD_ACT_RELU, d.z = fake(3); break;
        case 7: d.gate = fake(8), d.gate_act = GWD_ACT_RELU; break;
        case 8: d.gate = fake(8), d.gate_act = GWD_ACT_GELU; break;
        case 9:
        case 10:
            d.scale = (float *)fake(4), d.shift = (float *)fake(5), d.ln_mean = (float *)fake(9), d.ln_rstd = (float *)fake(10), d.ln_C = d.Cout;
            d.act = kind == 10 ? GWD_ACT_GELU : GWD_ACT_NONE;
            break;
        case 11: d.shift = (float *)fake(5), d.residual = fake(6), d.act = GWD_ACT_RELU; break;
        default: break;
    }
}

// input map (B, Hi, Wi), Cin -> Cout, square kernel k (pad k / 2 for odd k, else 0), stride s; the output size follows from the gather
gwd_conv_desc make_desc(int B, int Hi, int Wi, int Cin, int Cout, int k, int s, int gather, int dtype, bool zero_page = true) {
    gwd_conv_desc d;
    memset(&d, 0, sizeof d);
    d.x = fake(0), d.w = fake(1), d.y = fake(2);
    d.zero_page = zero_page ? fake(11) : nullptr;
    const int p = (k & 1) ? k / 2 : 0;
    d.B = B, d.Hi = Hi, d.Wi = Wi, d.Cin = Cin, d.Cout = Cout, d.KH = d.KW = k, d.stride = s, d.pad = p, d.gather = gather, d.dtype = dtype;
    d.act_scale = 1.0f;
    if (gather == GWD_GATHER_CONV) {
        d.Ho = (Hi + 2 * p - k) / s + 1, d.Wo = (Wi + 2 * p - k) / s + 1;
    } else if (gather == GWD_GATHER_TRANSPOSED) {         // the data gradient of that convolution: the map it read
        const int out_pad = (s == 2 && (k & 1)) ? 1 : 0;
        d.Ho = (Hi - 1) * s + k - 2 * p + out_pad, d.Wo = (Wi - 1) * s + k - 2 * p + out_pad;
    } else {                                               // 2x nearest up-sampling in front (stride 2 is refused by the library)
        d.Hv = 2 * Hi, d.Wv = 2 * Wi;
        d.Ho = d.Hv + 2 * p - k + 1, d.Wo = d.Wv + 2 * p - k + 1;
    }
    return d;
}

void put_desc(const gwd_conv_desc &d) {
    char buf[160];
    snprintf(buf, sizeof buf, " %dx%dx%dx%d>%dx%dx%d k%d s%d p%d g%d t%d", d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.Cout, d.KH, d.stride, d.pad, d.gather, d.dtype);
    g_line += buf;
}
void end_record(int rc) {
    // the launches were appended while the call ran; the return code goes in front of them
    const size_t bar = g_line.find(" | ");
    char buf[24];
    snprintf(buf, sizeof buf, " rc=%d", rc);
    g_line.insert(bar == std::string::npos ? g_line.size() : bar, buf);
    g_line += '\n';
    fwrite(g_line.data(), 1, g_line.size(), stdout);
    g_line.clear();
}

const int MAPS[][3] = {{8, 240, 320}, {8, 120, 160}, {8, 60, 80}, {8, 30, 40}, {8, 15, 20}, {2, 96, 128}, {2, 24, 32}, {800, 1, 1}, {2400, 1, 1}};
const int CHANNELS[] = {1, 2, 3, 8, 16, 24, 32, 48, 64, 80, 96, 128, 160, 256, 320, 1024, 2048};

template <class F> void for_each_shape(int dtype, F f) {
    for (const auto &m : MAPS)
        for (int cin : CHANNELS)
            for (int cout : CHANNELS)
                for (int k = 1; k <= 3; ++k)
                    for (int s = 1; s <= 2; ++s)
                        for (int g = 0; g < 3; ++g) f(make_desc(m[0], m[1], m[2], cin, cout, k, s, g, dtype));
}

void record_forward() {
    for (int dtype = GWD_BF16; dtype >= GWD_F32; --dtype)
        for (int kind = 0; kind < N_KINDS; ++kind) {
            printf("# forward %s %s\n", dtype == GWD_BF16 ? "bf16" : "f32", KINDS[kind]);
            for_each_shape(dtype, [&](gwd_conv_desc d) {
                set_epilogue(d, kind);
                g_line = "F";
                put_desc(d);
                end_record(gwd_conv_forward(&d, nullptr));
            });
        }
    // without a zero page (the register-staged kernels for bf16 as well), a few epilogues, one map
    printf("# forward no zero page\n");
    for (int kind : {0, 1, 4, 7, 8, 9})
        for (int cin : CHANNELS)
            for (int cout : CHANNELS)
                for (int k = 1; k <= 3; k += 2) {
                    gwd_conv_desc d = make_desc(8, 60, 80, cin, cout, k, 1, GWD_GATHER_CONV, GWD_BF16, false);
                    set_epilogue(d, kind);
                    g_line = "F";
                    put_desc(d);
                    g_line += " ";
                    g_line += KINDS[kind];
                    end_record(gwd_conv_forward(&d, nullptr));
                }
}

void record_wgrad(std::vector<gwd_conv_desc> &pool) {
    for (int dtype = GWD_BF16; dtype >= GWD_F32; --dtype)
        for (int scaled = 0; scaled < 2; ++scaled) {
            printf("# wgrad %s%s\n", dtype == GWD_BF16 ? "bf16" : "f32", scaled ? " scaled" : "");
            for_each_shape(dtype, [&](gwd_conv_desc d) {
                if (scaled) d.scale = (float *)fake(4);
                g_line = "W";
                put_desc(d);
                const int rc = gwd_conv_wgrad(&d, (float *)fake(12), nullptr);
                end_record(rc);
                if (rc == 0 && !scaled) pool.push_back(d);
            });
        }
    printf("# wgrad no zero page\n");                      // the register-staged kernels for bf16 as well
    for (int cin : CHANNELS)
        for (int cout : CHANNELS)
            for (int k = 1; k <= 3; k += 2) {
                gwd_conv_desc d = make_desc(8, 60, 80, cin, cout, k, 1, GWD_GATHER_CONV, GWD_BF16, false);
                g_line = "W";
                put_desc(d);
                const int rc = gwd_conv_wgrad(&d, (float *)fake(12), nullptr);
                end_record(rc);
                if (rc == 0) pool.push_back(d);
            }
}

// batches of mixed shapes drawn from every valid weight-gradient descriptor above (both dtypes), of 1 ... 67 jobs, and batches of 40 and
// 16 jobs of ONE shape for each of a few layers: the grouping by tile and gather form, the flush of a full group of 16 and the final flush
void record_wgrad_batch(const std::vector<gwd_conv_desc> &pool) {
    printf("# wgrad batch\n");
    std::vector<gwd_conv_desc> descs;
    std::vector<float *> dws;
    auto run = [&]() {
        char buf[32];
        snprintf(buf, sizeof buf, "B n=%d", (int)descs.size());
        g_line = buf;
        for (const gwd_conv_desc &d : descs) put_desc(d);
        end_record(gwd_conv_wgrad_batch(descs.data(), dws.data(), (int)descs.size(), nullptr));
        descs.clear(), dws.clear();
    };
    size_t pos = 0, stride = 7919;                        // a prime stride: neighbours in the walk differ in every field
    for (int b = 0; b < 6000; ++b) {
        const int n = 1 + (b * 13) % 67;
        for (int i = 0; i < n; ++i, pos = (pos + stride) % pool.size()) descs.push_back(pool[pos]), dws.push_back((float *)fake(12 + i % 4));
        run();
    }
    for (int b = 0; b < 400; ++b) {
        const gwd_conv_desc &d = pool[(b * 104729ull) % pool.size()];
        for (int n : {40, 16}) {
            for (int i = 0; i < n; ++i) descs.push_back(d), dws.push_back((float *)fake(12));
            run();
        }
    }
}

void record_weight_copies() {
    printf("# weight copies\n");
    for (int dtype = GWD_BF16; dtype >= GWD_F32; --dtype)
        for (int n : {8, 160, 2048}) {
            char buf[64];
            snprintf(buf, sizeof buf, "P N=%d taps=9 C=64 t%d", n, dtype);
            g_line = buf;
            end_record(gwd_weight_prep((const float *)fake(0), nullptr, fake(1), fake(2), n, 9, 64, dtype, nullptr));
        }
    g_line = "PB jobs=3 blocks=77";
    end_record(gwd_weight_prep_batch((const gwd_prep_job *)fake(0), 3, 77, nullptr, nullptr));
    gwd_unpad_job jobs[2];
    memset(jobs, 0, sizeof jobs);
    for (int i = 0; i < 2; ++i) jobs[i].src = (const float *)fake(0), jobs[i].dst = (float *)fake(1), jobs[i].N = 30 * (i + 1), jobs[i].taps = 9, jobs[i].G = 1, jobs[i].Cg = 30, jobs[i].Cgp = 32;
    g_line = "U jobs=2";
    end_record(gwd_unpad_add_batch(jobs, 2, nullptr));
}

// one call per input line, see the head of the file; a malformed line ends the run with status 2
int replay_stdin() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        char call = 0;
        int n = 1, v[10], a = 0, b = 0, as = 0, used = 0;
        if (line[0] == '#' || line[0] == '\n') continue;
        if (sscanf(line, " %c%n", &call, &used) != 1) return 2;
        const char *p = line + used;
        if (call == 'B') {
            if (sscanf(p, "%d%n", &n, &used) != 1 || n < 1 || n > 64) return 2;
            p += used;
        }
        for (int i = 0; i < 10; ++i) {
            if (sscanf(p, "%d%n", &v[i], &used) != 1) return 2;
            p += used;
        }
        if (call == 'F' && sscanf(p, "%d %d %d", &a, &b, &as) != 3) return 2;
        if ((call == 'W' || call == 'B') && sscanf(p, "%d", &a) != 1) return 2;
        gwd_conv_desc d = make_desc(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9] != 0);
        char buf[48];
        if (call == 'F') {
            if (a < 0 || a >= N_KINDS) return 2;
            set_epilogue(d, a);
            if (d.ln_mean && b > 0) d.ln_C = b;
            if (as) d.act_scale = 0.7f;
            g_line = "F";
            put_desc(d);
            snprintf(buf, sizeof buf, " %s zp=%d lnC=%d as=%d", KINDS[a], v[9] != 0, d.ln_C, as != 0);
            g_line += buf;
            end_record(gwd_conv_forward(&d, nullptr));
        } else if (call == 'W') {
            if (a) d.scale = (float *)fake(4);
            g_line = "W";
            put_desc(d);
            snprintf(buf, sizeof buf, " scaled=%d zp=%d", a != 0, v[9] != 0);
            g_line += buf;
            end_record(gwd_conv_wgrad(&d, (float *)fake(12), nullptr));
        } else if (call == 'B') {
            std::vector<gwd_conv_desc> descs;
            std::vector<float *> dws;
            snprintf(buf, sizeof buf, "B n=%d", n);
            g_line = buf;
            for (int i = 0; i < n; ++i) {
                descs.push_back(make_desc(v[0] + i, v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9] != 0));
                if (a) descs.back().scale = (float *)fake(4);
                dws.push_back((float *)fake(12 + i));
                put_desc(descs.back());
            }
            snprintf(buf, sizeof buf, " scaled=%d zp=%d", a != 0, v[9] != 0);
            g_line += buf;
            end_record(gwd_conv_wgrad_batch(descs.data(), dws.data(), n, nullptr));
        } else {
            return 2;
        }
    }
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    static char out_buf[1 << 20];
    setvbuf(stdout, out_buf, _IOFBF, sizeof out_buf);
    g_int_args = INT_ARGS, g_n_int_args = (int)(sizeof INT_ARGS / sizeof INT_ARGS[0]);
    if (argc > 1) return strcmp(argv[1], "--stdin") == 0 ? replay_stdin() : 2;
    record_forward();
    std::vector<gwd_conv_desc> pool;
    record_wgrad(pool);
    record_wgrad_batch(pool);
    record_weight_copies();
    return 0;
}
