// tests/c/dev_mem_test.cpp -- csrc/dev_mem.h, the ownership of device memory, as a stand-alone program for the sanitizer builds:
// the ops bound to malloc / free with a countdown that makes the k-th take fail -- what no GPU can be made to do.  A set that
// exists whole or not at all under every failing piece, adopt / swap / move, a set replaced on growth, a retry after a failure.
// AddressSanitizer's leak check at exit is the leak assertion.  No GPU call.
#include "dev_mem.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>

static int cases = 0, failures = 0;
static void check(bool ok, const char *what, int k)
{
    cases++;
    if (!ok) { failures++; printf("FAIL %s (k = %d)\n", what, k); }
}

static int fail_at = -1;       // the take that fails, counted down from here (negative: none)
static long live = 0;          // pieces taken and not given back
static long gives = 0, takes = 0;
static long live_at_take[64];  // live when take number i was asked for
static int t_take(void **out, size_t bytes)
{
    if (takes < 64) live_at_take[takes] = live;
    takes++;
    if (fail_at >= 0 && fail_at-- == 0) return -1;
    *out = malloc(bytes);
    live++;
    return 0;
}
static void t_give(void *p) { free(p); live--; gives++; }
static const AsxMemOps ops = { t_take, t_give };

// five pieces as the plan's float32 staging has them, one of them with a count of 0
struct Five {
    float *a = nullptr, *b = nullptr;
    int64_t *c = nullptr;
    double *d = nullptr;
    int32_t *e = nullptr;
    bool whole() const { return a && b && c && d && e; }
    bool absent() const { return !a && !b && !c && !d && !e; }
};
static const size_t five_bytes = 7 * 4 + 3 * 4 + 8 /* count 0: one element */ + 2 * 8 + 5 * 4;
static int fill_five(AsxMemSet &m, Five &t)
{
    return m.take(&t.a, 7) || m.take(&t.b, 3) || m.take(&t.c, 0) || m.take(&t.d, 2) || m.take(&t.e, 5) ? -1 : 0;
}

int main()
{
    // whole or absent: every failing piece k < 5, then none
    for (int k = 0; k <= 5; k++) {
        AsxMemSet owner(ops);
        char *mine = nullptr;
        check(owner.take(&mine, 10) == 0 && owner.bytes() == 10, "the owner's own piece", k);
        Five dst;
        fail_at = k < 5 ? k : -1;
        const long live0 = live;
        const int rc = asx_mem_whole(owner, dst, fill_five);
        fail_at = -1;
        if (k < 5) {
            check(rc == -1, "a failing piece fails the set", k);
            check(dst.absent(), "the destination is untouched", k);
            check(owner.bytes() == 10, "the owner's bytes are unchanged", k);
            check(live == live0, "nothing of the attempt is live", k);
            // the retry starts from nothing and ends with exactly one set
            check(asx_mem_whole(owner, dst, fill_five) == 0 && dst.whole(), "the retry succeeds", k);
            check(live == live0 + 5 && owner.bytes() == 10 + five_bytes, "one set live after the retry", k);
        } else {
            check(rc == 0 && dst.whole(), "every piece is set", k);
            check(owner.bytes() == 10 + five_bytes && live == live0 + 5, "the bytes add up", k);
            dst.a[6] = 1.f; dst.b[2] = 1.f; dst.c[0] = 1; dst.d[1] = 1.0; dst.e[4] = 1; // (each piece is as long as it says)
        }
        owner.clear();
        check(owner.bytes() == 0 && live == 0, "clear gives everything back", k);
    }
    // adopt, swap, move
    {
        AsxMemSet x(ops), y(ops);
        int *p = nullptr, *q = nullptr, *r = nullptr;
        check(!x.take(&p, 1) && !x.take(&q, 2) && !y.take(&r, 5), "takes", 0);
        x.swap(y);
        check(x.bytes() == 20 && y.bytes() == 12, "swap moves the bytes", 0);
        const long g0 = gives;
        y.clear();
        check(gives == g0 + 2 && live == 1, "swap moves the ownership", 0);
        r[4] = 7; // still x's
        check(!y.take(&p, 3), "take", 0);
        x.adopt(y);
        check(x.bytes() == 32 && y.bytes() == 0 && live == 2, "adopt moves bytes and ownership", 0);
        const long g1 = gives;
        y.clear();
        check(gives == g1, "an adopted set gives nothing back", 0);
        {
            AsxMemSet z(std::move(x));
            check(z.bytes() == 32 && x.bytes() == 0, "a move takes the bytes", 0);
            x.clear();
            check(gives == g1 && live == 2, "a moved-from set gives nothing back", 0);
        }
        check(gives == g1 + 2 && live == 0, "the moved-to set gives back once, by scope", 0);
    }
    // a set replaced on growth (the bank): the old pieces go before the new ones are asked for; a failed growth leaves it empty
    {
        AsxMemSet bank(ops);
        Five c;
        check(asx_mem_whole(bank, c, fill_five) == 0 && live == 5, "the first bank", 0);
        for (int k : { 2, -1 }) {
            bank.clear();
            c = Five{};
            const long t0 = takes;
            fail_at = k;
            const int rc = asx_mem_whole(bank, c, fill_five);
            fail_at = -1;
            check(t0 < 64 && live_at_take[t0] == 0, "the old bank is gone before the first new take", k);
            if (k >= 0) check(rc == -1 && c.absent() && bank.bytes() == 0 && live == 0, "a failed growth leaves the bank empty", k);
            else check(rc == 0 && c.whole() && bank.bytes() == five_bytes && live == 5, "the grown bank is the only one live", k);
        }
    }
    check(live == 0, "nothing is live at the end", 0);
    printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
