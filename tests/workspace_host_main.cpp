// Stand-alone check of csrc/workspace.h, built by tests/test_workspace_host.py with the host compiler and
// -fsanitize=address,undefined.  Exit status 0 = every check held; a failed check prints its line.
#include "workspace.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>

using xrs::Carver;
using xrs::up256;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

struct Odd { char c[13]; };                     // a size that is no power of two

struct Parts {
    uint64_t *a;
    unsigned char *b;
    Odd *c;
    uint32_t *none;                             // a count of 0
    void *word;                                 // 256 raw bytes
    double *d;
    void *raw;                                  // raw bytes that are no multiple of 256: taken as they are
    float *last;
    size_t before_last, total;
};

// the same sequence of takes sizes the block (null base) and carves it
static Parts carve(void *base, size_t n) {
    Carver c(base);
    Parts p = {};
    p.a = c.take<uint64_t>(n);
    p.b = c.take<unsigned char>(n);
    p.c = c.take<Odd>(n);
    p.none = c.take<uint32_t>(0);
    p.word = c.take_bytes(256);
    p.d = c.take<double>(n + 1);
    p.raw = c.take_bytes(512 + 40);
    p.before_last = c.at();
    p.last = c.take<float>(1);
    p.total = c.at();
    return p;
}

static bool aligned(const void *p) { return reinterpret_cast<uintptr_t>(p) % 256 == 0; }

int main() {
    CHECK(up256(0) == 0 && up256(1) == 256 && up256(255) == 256 && up256(256) == 256 && up256(257) == 512);
    CHECK(up256(((size_t)1 << 40) + 1) == ((size_t)1 << 40) + 256);

    const size_t sizes[] = {0, 1, 31, 32, 255, 256, 257, 4097};
    for (size_t n : sizes) {
        const Parts s = carve(nullptr, n);      // sizing pass: null pointers, and no arithmetic on the null pointer (UBSan)
        CHECK(!s.a && !s.b && !s.c && !s.none && !s.word && !s.d && !s.raw && !s.last);

        void *mem = nullptr;
        CHECK(posix_memalign(&mem, 256, s.total) == 0);
        char *block = static_cast<char *>(mem);
        const Parts p = carve(block, n);
        CHECK(p.total == s.total && p.before_last == s.before_last);

        // each pointer is the base plus the rounded sum of what came before it
        size_t at = 0;
        CHECK((char *)p.a == block + at); at += up256(n * 8);
        CHECK((char *)p.b == block + at); at += up256(n);
        CHECK((char *)p.c == block + at); at += up256(n * 13);
        CHECK((char *)p.none == block + at);    // a count of 0: the address of the next part, no bytes
        CHECK((char *)p.word == block + at); at += 256;
        CHECK((char *)p.d == block + at); at += up256((n + 1) * 8);
        CHECK((char *)p.raw == block + at); at += 552;           // raw bytes are not rounded ..
        CHECK((char *)p.last == block + at && p.before_last == at);   // .. so the next part starts right behind them
        at += 256;
        CHECK(p.total == at);
        CHECK(aligned(p.a) && aligned(p.b) && aligned(p.c) && aligned(p.none) && aligned(p.word) && aligned(p.d) && aligned(p.raw));

        // the last byte of every part lies inside the block (ASan)
        if (n) { p.a[n - 1] = 1; p.b[n - 1] = 1; p.c[n - 1].c[12] = 1; }
        static_cast<char *>(p.word)[255] = 1;
        p.d[n] = 1.0;
        static_cast<char *>(p.raw)[551] = 1;
        p.last[0] = 1.0f;
        block[p.total - 1] = 1;
        std::free(block);
    }
    if (failures) return 1;
    std::puts("workspace.h: ok");
    return 0;
}
