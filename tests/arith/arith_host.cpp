// arith_host.cpp -- the host pass of the arithmetic headers on a file of cases (see arith_ops.hpp): built with g++ and the flags of
// the product's host input builders.  The device-only entries (dw_math.hpp, the packed forms) are not in it; their cases come back
// as zeros and the tests do not look at them.
//   arith_host --list             prints "id name words_in words_out" per entry
//   arith_host cases.bin out.bin  evaluates
#include <stdio.h>
#include <string.h>

#include <vector>

#include "arith_ops.hpp"

using namespace arith;

#define ARITH_OPS_HOST(X) ARITH_OPS_HDR(X) ARITH_OPS_DF32(X) ARITH_OPS_QD(X) ARITH_OPS_BLA(X)

static void eval(const uint32_t *p, uint32_t *o)
{
    switch (*p++) {
        ARITH_OPS_HOST(ARITH_CASE)
    default:
        break;
    }
}

#define ARITH_LIST(id, name, TA, TB, TC, expr)                                                                            \
    {                                                                                                                     \
        TA a;                                                                                                             \
        TB b;                                                                                                             \
        TC c;                                                                                                             \
        (void)sizeof(a), (void)sizeof(b), (void)sizeof(c);                                                                \
        printf("%d %s %d %d\n", (int)(id), #name, words<TA>::n + words<TB>::n + words<TC>::n, words<decltype(expr)>::n);  \
    }

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "--list")) {
        ARITH_OPS_HOST(ARITH_LIST)
        return 0;
    }
    if (argc != 3) {
        fprintf(stderr, "usage: arith_host --list | arith_host cases.bin out.bin\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 3;
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1)
        return 3;
    std::vector<uint32_t> in((size_t)n * kCaseWords), out((size_t)n * kOutWords, 0u);
    if (n && fread(in.data(), 4, in.size(), f) != in.size())
        return 3;
    fclose(f);
    for (uint32_t i = 0; i < n; ++i)
        eval(&in[(size_t)i * kCaseWords], &out[(size_t)i * kOutWords]);
    f = fopen(argv[2], "wb");
    if (!f || (n && fwrite(out.data(), 4, out.size(), f) != out.size()) || fclose(f) != 0)
        return 4;
    return 0;
}
