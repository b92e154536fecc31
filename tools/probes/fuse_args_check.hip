// Host-side check of urso_pose_fuse_views' argument validation under the address and undefined-behaviour sanitizers, without a GPU: a
// stand-alone program (the extension's source compiled into it, the main library's error plumbing replaced by the few lines below) that
// walks every refusal of include/ursonet_ext.h and the n = 0 case.  Nothing is launched and no device pointer is dereferenced.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/probes/fuse_args_check.hip -o tools/probes/bin/fuse_args_check && tools/probes/bin/fuse_args_check
#include "../../ursonet_amd/csrc_ext/pose_fuse.hip"
#include <stdarg.h>
#include <string.h>

static char g_err[512];
void urso_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
int urso_check_launch(const char*) { return URSO_ELAUNCH; }               // reaching a launch is a failure of this program
void urso_prof_before(hipStream_t, int, double, double) {}
void urso_prof_after(hipStream_t) {}
void urso_prof_symbol(const void*) {}

static urso_pose_fuse_views_args good() {
    urso_pose_fuse_views_args a;
    memset(&a, 0, sizeof a);
    a.B = 4; a.n = 4; a.row0 = 0; a.V = 3; a.est_ld = 12; a.est_view_rows = 4;
    a.est = a.r = a.qr = (const double*)4096; a.table = (double*)4096;     // never dereferenced
    return a;
}

static int failures = 0;
static void refuse(const char* what, const urso_pose_fuse_views_args* a, const char* needle) {
    g_err[0] = 0;
    const int rc = urso_pose_fuse_views(a, nullptr);
    if (rc != URSO_EINVAL || strncmp(g_err, "urso_pose_fuse_views:", 21) != 0 || !strstr(g_err, needle)) {
        printf("FAIL %s: rc %d, error '%s'\n", what, rc, g_err);
        ++failures;
    }
}

int main() {
    urso_pose_fuse_views_args a;
    refuse("null struct", nullptr, "null");
    a = good(); a.est = nullptr; refuse("null est", &a, "null");
    a = good(); a.r = nullptr; refuse("null r", &a, "null");
    a = good(); a.qr = nullptr; refuse("null qr", &a, "null");
    a = good(); a.table = nullptr; refuse("null table", &a, "null");
    a = good(); a.loc_gt = (const double*)4096; refuse("loc_gt alone", &a, "both or neither");
    a = good(); a.q_gt = (const double*)4096; refuse("q_gt alone", &a, "both or neither");
    a = good(); a.B = 0; a.n = 0; refuse("B = 0", &a, "B > 0");
    a = good(); a.B = INT32_MIN; a.n = 0; refuse("B = INT32_MIN", &a, "B > 0");
    a = good(); a.n = 5; refuse("n > B", &a, "n <= B");
    a = good(); a.n = -1; refuse("n < 0", &a, "n <= B");
    a = good(); a.row0 = -1; refuse("row0 < 0", &a, "row0");
    a = good(); a.row0 = INT64_MIN; refuse("row0 = INT64_MIN", &a, "row0");
    a = good(); a.V = 0; refuse("V = 0", &a, "V");
    a = good(); a.V = 65; refuse("V = 65", &a, "V");
    a = good(); a.V = INT32_MAX; refuse("V = INT32_MAX", &a, "V");
    a = good(); a.est_ld = 6; refuse("est_ld = 6", &a, "est_ld");
    a = good(); a.est_ld = INT32_MIN; refuse("est_ld = INT32_MIN", &a, "est_ld");
    a = good(); a.est_view_rows = 3; refuse("est_view_rows < B", &a, "est_view_rows");
    a = good(); a.est_view_rows = INT64_MIN; refuse("est_view_rows = INT64_MIN", &a, "est_view_rows");
    a = good(); a.n = 0;
    if (urso_pose_fuse_views(&a, nullptr) != URSO_OK) { printf("FAIL n = 0 is valid and launches nothing\n"); ++failures; }
    a.loc_gt = a.q_gt = (const double*)4096; a.V = 64; a.est_ld = 7; a.row0 = INT64_MAX;
    if (urso_pose_fuse_views(&a, nullptr) != URSO_OK) { printf("FAIL n = 0 with a truth\n"); ++failures; }
    printf(failures ? "fuse_args_check: %d FAILED\n" : "fuse_args_check OK\n", failures);
    return failures ? 1 : 0;
}
