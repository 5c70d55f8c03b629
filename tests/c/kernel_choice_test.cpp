// tests/c/kernel_choice_test.cpp -- csrc/plan_math.cpp's host plans and the kernels they resolve to (AsxKernelChoice against the
// lists of csrc/kernel_table.h), as a stand-alone program for the sanitizer builds: the six production lengths and the lengths
// and splits outside the table, under the default environment, ASX_LAYOUT=packed and ASX_GENERIC=1.  No GPU call.
#include "plan_math.h"
#include "kernel_table.h"

#include <cstdio>
#include <cstdlib>

static int cases = 0, failures = 0;
static void check(bool ok, const char *what, size_t n, const char *env)
{
    cases++;
    if (!ok) { failures++; printf("FAIL %s (n = %zu, %s)\n", what, n, env); }
}

static void one(size_t n, const char *split, const char *env, int want_real, bool want_entries)
{
    AsxHostPlan h;
    const std::string err = asx_host_plan_build(n, split, &h);
    check(err.empty(), "plan", n, env);
    if (!err.empty()) return;
    const AsxKernelChoice &k = h.kernels;
    int cols[ASX_ENTRY_INTS], rows[ASX_ENTRY_INTS];
    asx_kernel_table_spell(k.rlayout ? 0 : 2, k.cols, cols);
    asx_kernel_table_spell(k.rlayout ? 1 : 3, k.rows, rows);
    check(k.rlayout == (want_real != 0), "layout", n, env);
    check((k.cols >= 0) == want_entries && (k.rows >= 0) == want_entries, "entries", n, env);
    check((cols[0] >= 0) == want_entries && (rows[0] >= 0) == want_entries, "spelling", n, env);
    if (k.rlayout) {
        check(cols[0] == h.M1 && cols[1] == h.T && k.band_rows > 0 && 2 * h.M1 % k.band_rows == 0, "real-column columns", n, env);
        check(rows[2] * (rows[1] ? 2 : 1) == h.M2, "real-column rows", n, env);
    } else if (want_entries) {
        check(cols[0] == h.M1 && cols[1] == h.T && cols[2] == k.threads_cols, "packed columns", n, env);
        check(rows[2] == h.M2 && rows[0] == k.threads_rows, "packed rows", n, env);
    }
    // a spelled entry ends its radices with a 0 inside the buffer, and they multiply to the transform length
    for (const int *e : { cols, rows }) {
        if (e[0] < 0) continue;
        const int nhead = (!k.rlayout && e == cols) ? 4 : 3;
        long prod = 1;
        int i = nhead;
        while (i < ASX_ENTRY_INTS && e[i]) prod *= e[i++];
        check(i < ASX_ENTRY_INTS && prod == (e == cols ? e[0] : e[2]), "radices", n, env);
    }
}

int main()
{
    const size_t production[] = { 144000, 288000, 480000, 720000, 960000, 1440000 };
    const struct { const char *name, *value; int real; bool entries; } envs[] = {
        { nullptr, nullptr, 1, true }, { "ASX_LAYOUT", "packed", 0, true }, { "ASX_GENERIC", "1", 0, false } };
    for (const auto &e : envs) {
        unsetenv("ASX_LAYOUT");
        unsetenv("ASX_GENERIC");
        if (e.name) setenv(e.name, e.value, 1);
        const char *label = e.name ? e.name : "default";
        for (size_t n : production) one(n, "", label, e.real, e.entries);
        for (size_t n : { (size_t)1, (size_t)7, (size_t)1000, (size_t)12345 }) one(n, "", label, 0, false);
        one(1000, "25x40x8", label, 0, false);
        one(144000, "150x960x16", label, 0, false);
        AsxHostPlan h;
        check(!asx_host_plan_build(144000, "1x144000x1", &h).empty(), "a split without a column pair is refused", 144000, label);
    }
    printf("%d cases, %d failures\n", cases, failures);
    return failures != 0;
}
