// Host check of csrc/dev_buf.h: DevBuf and dev_ensure_all against link-time fakes of hipMalloc / hipFree over malloc / free
// that count calls, keep a live-block count and fail on demand.  No HIP runtime is linked.  tests/test_dev_buf_host.py builds
// this with the host compiler under -fsanitize=address,undefined and wants exit status 0.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "../../global-motion-estimation_amd/csrc/dev_buf.h"

static int g_mallocs = 0, g_frees = 0, g_live = 0;
static int g_fail_at = 0;                 // the g_fail_at-th hipMalloc from now fails (0: none)
static std::vector<char> g_order;         // 'm' / 'f' per allocator call
static char g_err[512] = "";

extern "C" hipError_t hipMalloc(void** p, size_t bytes)
{
    ++g_mallocs;
    g_order.push_back('m');
    if (g_fail_at > 0 && --g_fail_at == 0) { *p = (void*)(uintptr_t)0xdead; return hipErrorOutOfMemory; }
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return hipErrorOutOfMemory;
    memset(*p, 0xA5, bytes);              // the whole block is ours to write
    ++g_live;
    return hipSuccess;
}

extern "C" hipError_t hipFree(void* p)
{
    ++g_frees;
    g_order.push_back('f');
    if (p) { free(p); --g_live; }
    return hipSuccess;
}

void gme_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int g_failed = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

static int calls() { return g_mallocs + g_frees; }

static void single_buffer()
{
    DevBuf<double> b;
    CHECK(b.get() == nullptr && b.cap == 0);
    CHECK(b.ensure(0, "nothing") == GME_OK && calls() == 0 && b.get() == nullptr);      // ensure(0) leaves it as it is

    CHECK(b.ensure(100, "rows") == GME_OK);
    CHECK(b.get() != nullptr && b.cap == 100 && g_mallocs == 1 && g_frees == 0 && g_live == 1);
    double* first = b.get();
    CHECK((double*)b == first);

    // reuse: no allocator call at or below the capacity, ensure(0) included
    int before = calls();
    CHECK(b.ensure(100, "rows") == GME_OK && b.ensure(7, "rows") == GME_OK && b.ensure(0, "rows") == GME_OK);
    CHECK(calls() == before && b.get() == first && b.cap == 100);

    // growth: the old block is freed before the new one is asked for
    g_order.clear();
    CHECK(b.ensure(101, "rows") == GME_OK);
    CHECK(g_order.size() == 2 && g_order[0] == 'f' && g_order[1] == 'm');
    CHECK(b.cap == 101 && g_live == 1);

    // a failed allocation: empty, GME_ERR_NOMEM, a text with the name and the byte count
    g_fail_at = 1;
    g_err[0] = 0;
    CHECK(b.ensure(1000, "summary rows") == GME_ERR_NOMEM);
    CHECK(b.get() == nullptr && b.cap == 0 && g_live == 0);
    CHECK(strstr(g_err, "summary rows") != nullptr && strstr(g_err, std::to_string(1000 * sizeof(double)).c_str()) != nullptr);
    CHECK(strstr(g_err, "out of device memory") != nullptr);

    // ... and the retry allocates again
    before = g_mallocs;
    CHECK(b.ensure(1000, "summary rows") == GME_OK && g_mallocs == before + 1 && b.cap == 1000 && g_live == 1);

    // n * sizeof(T) past size_t: GME_ERR_NOMEM without any allocator call, so a held block stays as it is
    before = calls();
    g_err[0] = 0;
    double* held = b.get();
    CHECK(b.ensure((size_t)-1 / sizeof(double) + 1, "too much") == GME_ERR_NOMEM);
    CHECK(calls() == before && b.get() == held && b.cap == 1000 && g_live == 1 && strstr(g_err, "too much") != nullptr);
    DevBuf<double> fresh;
    CHECK(fresh.ensure((size_t)-1 / 2, "too much") == GME_ERR_NOMEM && calls() == before && fresh.get() == nullptr && fresh.cap == 0);

    // reset() and the destructor
    CHECK(b.ensure(5, "rows") == GME_OK && g_live == 1);
    b.reset();
    CHECK(b.get() == nullptr && b.cap == 0 && g_live == 0);
    before = calls();
    b.reset();
    CHECK(calls() == before);                                // nothing to free
    {
        DevBuf<uint8_t> scoped;
        CHECK(scoped.ensure(33, "bytes") == GME_OK && g_live == 1);
    }
    CHECK(g_live == 0);

    // moves hand the block over, once
    DevBuf<int32_t> a;
    CHECK(a.ensure(9, "field") == GME_OK);
    int32_t* pa = a.get();
    DevBuf<int32_t> c(std::move(a));
    CHECK(a.get() == nullptr && a.cap == 0 && c.get() == pa && c.cap == 9 && g_live == 1);
    DevBuf<int32_t> d;
    CHECK(d.ensure(3, "field") == GME_OK && g_live == 2);
    d = std::move(c);
    CHECK(d.get() == pa && d.cap == 9 && c.get() == nullptr && g_live == 1);
    d = DevBuf<int32_t>();
    CHECK(d.get() == nullptr && g_live == 0);
}

static void groups()
{
    // every member large enough
    {
        DevBuf<uint8_t> x;
        DevBuf<double> y;
        DevBuf<unsigned long long> z;
        CHECK(dev_ensure_all("group", { { x, 10 }, { y, 20 }, { z, 30 } }) == GME_OK);
        CHECK(x.cap == 10 && y.cap == 20 && z.cap == 30 && g_live == 3);
        const int before = calls();
        CHECK(dev_ensure_all("group", { { x, 10 }, { y, 2 }, { z, 0 } }) == GME_OK && calls() == before);
    }
    CHECK(g_live == 0);
    // the k-th of three allocations fails: all three end empty, whether they were empty before or held a smaller block
    for (int held = 0; held <= 1; ++held)
        for (int k = 1; k <= 3; ++k) {
            DevBuf<uint8_t> x;
            DevBuf<double> y;
            DevBuf<unsigned long long> z;
            if (held) CHECK(dev_ensure_all("group", { { x, 1 }, { y, 1 }, { z, 1 } }) == GME_OK && g_live == 3);
            g_fail_at = k;
            g_err[0] = 0;
            CHECK(dev_ensure_all("group", { { x, 10 }, { y, 20 }, { z, 30 } }) == GME_ERR_NOMEM);
            g_fail_at = 0;
            CHECK(x.get() == nullptr && y.get() == nullptr && z.get() == nullptr && x.cap == 0 && y.cap == 0 && z.cap == 0);
            CHECK(g_live == 0 && strstr(g_err, "group") != nullptr);
            // the retry allocates all three again
            const int before = g_mallocs;
            CHECK(dev_ensure_all("group", { { x, 10 }, { y, 20 }, { z, 30 } }) == GME_OK && g_mallocs == before + 3 && g_live == 3);
        }
    CHECK(g_live == 0);
}

int main()
{
    single_buffer();
    groups();
    CHECK(g_live == 0);
    CHECK(g_mallocs > 0 && g_frees > 0);
    if (g_failed) { printf("dev_buf_check: %d checks failed\n", g_failed); return 1; }
    printf("dev_buf_check ok: %d allocations, %d frees, none live\n", g_mallocs, g_frees);
    return 0;
}
