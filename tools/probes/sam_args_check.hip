// Host-side check of the argument validation of urso_sam_ascend / urso_sam_descend / urso_sam_settle under the address and
// undefined-behaviour sanitizers, without a GPU: a stand-alone program (the library's source compiled into it, the main library's error
// plumbing replaced by the few lines below) that walks every refusal of include/ursonet_train.h and the n = 0 case.  Nothing is launched
// and no device pointer is dereferenced.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/probes/sam_args_check.hip -o tools/probes/bin/sam_args_check && tools/probes/bin/sam_args_check
#include "../../ursonet_amd/csrc_train/sam.hip"
#include <stdarg.h>
#include <string.h>

static char g_err[512];
void urso_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
int urso_check_launch(const char*) { return URSO_ELAUNCH; }               // reaching a launch is a failure of this program
void urso_prof_before(hipStream_t, int, double, double) {}
void urso_prof_after(hipStream_t) {}
void urso_prof_symbol(const void*) {}

static int failures = 0;
static void refused(const char* fn, const char* what, int rc, const char* needle) {
    if (rc != URSO_EINVAL || strncmp(g_err, fn, strlen(fn)) != 0 || g_err[strlen(fn)] != ':' || !strstr(g_err, needle)) {
        printf("FAIL %s %s: rc %d, error '%s'\n", fn, what, rc, g_err);
        ++failures;
    }
    g_err[0] = 0;
}
static void accepted(const char* what, int rc) {
    if (rc != URSO_OK) { printf("FAIL %s: rc %d, error '%s'\n", what, rc, g_err); ++failures; }
}

int main() {
    float* const W = (float*)0x10000; float* const G = (float*)0x20000; float* const W0 = (float*)0x30000;      // never dereferenced
    float* const ST = (float*)0x40000; float* const NSQ = (float*)0x50000;
    auto off = [](float* p, int bytes) { return (float*)((uintptr_t)p + bytes); };
    const char* A = "urso_sam_ascend";
    refused(A, "null w", urso_sam_ascend(1000, nullptr, G, W0, ST, nullptr), "null");
    refused(A, "null g", urso_sam_ascend(1000, W, nullptr, W0, ST, nullptr), "null");
    refused(A, "null w0", urso_sam_ascend(1000, W, G, nullptr, ST, nullptr), "null");
    refused(A, "null state", urso_sam_ascend(1000, W, G, W0, nullptr, nullptr), "null");
    refused(A, "n = -1", urso_sam_ascend(-1, W, G, W0, ST, nullptr), "n must be >= 0");
    refused(A, "n = INT64_MIN", urso_sam_ascend(INT64_MIN, W, G, W0, ST, nullptr), "n must be >= 0");
    refused(A, "w + 2", urso_sam_ascend(1000, off(W, 2), G, W0, ST, nullptr), "4-byte aligned");
    refused(A, "g + 1", urso_sam_ascend(1000, W, off(G, 1), W0, ST, nullptr), "4-byte aligned");
    refused(A, "w0 + 3", urso_sam_ascend(1000, W, G, off(W0, 3), ST, nullptr), "4-byte aligned");
    refused(A, "state + 2", urso_sam_ascend(1000, W, G, W0, off(ST, 2), nullptr), "4-byte aligned");
    refused(A, "g = w", urso_sam_ascend(1000, W, W, W0, ST, nullptr), "three buffers");
    refused(A, "w0 = w", urso_sam_ascend(1000, W, G, W, ST, nullptr), "three buffers");
    refused(A, "w0 = g", urso_sam_ascend(1000, W, G, G, ST, nullptr), "three buffers");
    refused(A, "one buffer, n = 0", urso_sam_ascend(0, W, W, W, ST, nullptr), "three buffers");
    accepted("ascend n = 0", urso_sam_ascend(0, W, G, W0, ST, nullptr));
    accepted("ascend n = 0, three alignments", urso_sam_ascend(0, off(W, 4), off(G, 8), off(W0, 12), ST, nullptr));
    const char* D = "urso_sam_descend";
    refused(D, "null w", urso_sam_descend(1000, nullptr, W0, nullptr), "null");
    refused(D, "null w0", urso_sam_descend(1000, W, nullptr, nullptr), "null");
    refused(D, "n = -1", urso_sam_descend(-1, W, W0, nullptr), "n must be >= 0");
    refused(D, "n = INT64_MIN", urso_sam_descend(INT64_MIN, W, W0, nullptr), "n must be >= 0");
    refused(D, "w + 2", urso_sam_descend(1000, off(W, 2), W0, nullptr), "4-byte aligned");
    refused(D, "w0 + 1", urso_sam_descend(1000, W, off(W0, 1), nullptr), "4-byte aligned");
    refused(D, "w0 = w", urso_sam_descend(1000, W, W, nullptr), "same buffer");
    accepted("descend n = 0", urso_sam_descend(0, W, W0, nullptr));
    accepted("descend n = 0, two alignments", urso_sam_descend(0, off(W, 4), W0, nullptr));
    const char* S = "urso_sam_settle";
    refused(S, "null state", urso_sam_settle(nullptr, NSQ, 1, nullptr), "null");
    refused(S, "null normsq", urso_sam_settle(ST, nullptr, 1, nullptr), "null");
    refused(S, "state + 2", urso_sam_settle(off(ST, 2), NSQ, 1, nullptr), "4-byte aligned");
    refused(S, "normsq + 1", urso_sam_settle(ST, off(NSQ, 1), 0, nullptr), "4-byte aligned");
    refused(S, "guard = 2", urso_sam_settle(ST, NSQ, 2, nullptr), "guard");
    refused(S, "guard = INT32_MIN", urso_sam_settle(ST, NSQ, INT32_MIN, nullptr), "guard");
    // the split of the walk is host arithmetic too: the vectors only where all three buffers sit alike, never more elements than n
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b)
            for (int c = 0; c < 4; ++c)
                for (size_t n : {(size_t)1, (size_t)3, (size_t)4, (size_t)5, (size_t)1025, (size_t)1 << 40}) {
                    const FlatSplit s = flat_split(n, off(W, 4 * a), off(G, 4 * b), off(W0, 4 * c));
                    const bool alike = a == b && b == c;
                    const size_t head = alike ? (size_t)((4 - a) & 3) : n;
                    const bool ok = alike ? (s.head == (head < n ? head : n) && s.nvec == (n - s.head) / 4) : (s.head == n && s.nvec == 0);
                    if (!ok || s.head + 4 * s.nvec > n) { printf("FAIL flat_split %d %d %d n %zu: head %zu nvec %zu\n", a, b, c, n, s.head, s.nvec); ++failures; }
                    const FlatSplit two = flat_split(n, off(W, 4 * a), off(G, 4 * b));
                    if (a == b && c == a && (two.head != s.head || two.nvec != s.nvec)) { printf("FAIL flat_split of two differs\n"); ++failures; }
                }
    printf(failures ? "sam_args_check: %d FAILED\n" : "sam_args_check OK\n", failures);
    return failures ? 1 : 0;
}
