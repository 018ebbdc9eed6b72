// Host test of athena_amd/csrc/pieces.h (tests/test_pieces.py compiles and runs it, under the address and undefined-behaviour
// sanitizers where they link).  Part one carves arrays of every element size and of the counts round a 256-byte boundary out of a
// std::vector<char> and writes every byte of every piece.  Part two holds bytes() to the arithmetic the four carvers of the library
// had before pieces.h, `total += (bytes + 255) & ~255` per piece, on the lists of contraction, top-k, grid clusters and the sampler.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pieces.h"

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

namespace {

struct S32 {
    char b[32];
};

// pointers of one element type, and what was asked of each
struct Asked {
    void *p;         // the T * that place() writes
    size_t bytes;    // count * sizeof(T)
};
template <typename T> struct Arrays {
    T *p[16] = {};
    int n = 0;
    void add(amp::Pieces &pc, std::vector<Asked> &asked, size_t count)
    {
        CHECK(n < 16);
        pc.add(&p[n], count);
        asked.push_back(Asked{&p[n], count * sizeof(T)});
        ++n;
    }
};

void carve_and_write()
{
    amp::Pieces pc;
    std::vector<Asked> asked;
    Arrays<uint8_t> a1;
    Arrays<uint32_t> a4;
    Arrays<uint64_t> a8;
    Arrays<S32> a32;
    const size_t counts[5] = {0, 1, 63, 64, 65};
    for (size_t c : counts) {                                          // 64 * 4 and 32 * 8 are exactly one unit
        a1.add(pc, asked, c);
        a4.add(pc, asked, c);
        a8.add(pc, asked, c);
        a32.add(pc, asked, c);
    }
    a8.add(pc, asked, 31), a8.add(pc, asked, 32), a8.add(pc, asked, 33);
    a32.add(pc, asked, 7), a32.add(pc, asked, 8), a32.add(pc, asked, 9);
    a1.add(pc, asked, 255), a1.add(pc, asked, 256), a1.add(pc, asked, 257);
    a1.add(pc, asked, 0);                                              // a last piece of nothing: base + bytes()

    const size_t total = pc.bytes();
    std::vector<char> store(total);
    char *base = store.data();
    pc.place(base);
    size_t end_of_last = 0;
    for (size_t i = 0; i < asked.size(); ++i) {
        char *at = nullptr;
        memcpy(&at, asked[i].p, sizeof(at));
        CHECK(at >= base && at <= base + total);                       // a piece of nothing included
        const size_t off = (size_t)(at - base);
        CHECK(off % 256 == 0);
        CHECK(off >= end_of_last);                                     // in the order of add(), none on top of another
        CHECK(off + asked[i].bytes <= total);
        end_of_last = off + asked[i].bytes;
        memset(at, (int)(i + 1), asked[i].bytes);
    }
    for (size_t i = 0; i < asked.size(); ++i) {                        // every byte still its owner's
        char *at = nullptr;
        memcpy(&at, asked[i].p, sizeof(at));
        for (size_t b = 0; b < asked[i].bytes; ++b) CHECK(at[b] == (char)(i + 1));
    }
    a4.p[1][0] = 7u, a8.p[2][62] = 9u;                                  // and usable as what they were declared
    CHECK(a4.p[1][0] == 7u && a8.p[2][62] == 9u);

    amp::Pieces none;
    CHECK(none.bytes() == 0);
    none.place(nullptr);
}

// the arithmetic of the carvers before pieces.h
struct Old {
    size_t total = 0;
    void piece(size_t bytes) { total += (bytes + 255) & ~(size_t)255; }
};

// stand-ins for scan64::tiles and radix::scratch_bytes: both sides of a comparison get the same number
size_t tiles(size_t n) { return (n + 2047) / 2048; }
size_t sort_scratch(size_t n) { return 4 * (256 * ((n + 4095) / 4096) + 256); }

struct Info {
    unsigned long long w[4];
};
struct Grid {
    float lo[3], inv_w[3];
    int32_t nc[3];
};
typedef unsigned long long u64;

void contraction(size_t E)
{
    Old o;
    o.piece(sizeof(Info)), o.piece(8 * E), o.piece(8 * E), o.piece(8 * E), o.piece(8 * E), o.piece(8 * (tiles(E) + 1)), o.piece(4 * E);
    o.piece(4 * E), o.piece(4 * E), o.piece(4 * (E + 1)), o.piece(4 * 4 * 512), o.piece(sort_scratch(E));
    Info *info;
    u64 *key, *key_s, *key_t, *before, *tile;
    int32_t *perm, *perm_t, *start, *longest;
    uint32_t *flag;
    char *temp;
    amp::Pieces pc;
    pc.add(&info, 1), pc.add(&key, E), pc.add(&key_s, E), pc.add(&key_t, E), pc.add(&before, E), pc.add(&tile, tiles(E) + 1), pc.add(&perm, E);
    pc.add(&perm_t, E), pc.add(&flag, E), pc.add(&start, E + 1), pc.add(&longest, 4 * 512), pc.add(&temp, sort_scratch(E));
    CHECK(pc.bytes() == o.total);
}

void topk(size_t n, size_t ns, size_t B)
{
    Old o;
    o.piece(8 * n), o.piece(8 * (tiles(n) + 1)), o.piece(8 * ns), o.piece(8 * ns), o.piece(8 * ns), o.piece(4 * ns), o.piece(4 * ns);
    o.piece(4 * ns), o.piece(4 * n), o.piece(4 * n), o.piece(4 * (B + 1)), o.piece(4 * B), o.piece(4 * B), o.piece(4 * (B + 1));
    o.piece(ns > 0 ? sort_scratch(ns) : 0);
    u64 *before, *tile, *key, *key_s, *key_t;
    int32_t *val, *val_s, *val_t, *rank, *off, *gpos, *k, *soff;
    uint32_t *flag;
    char *temp;
    amp::Pieces pc;
    pc.add(&before, n), pc.add(&tile, tiles(n) + 1), pc.add(&key, ns), pc.add(&key_s, ns), pc.add(&key_t, ns), pc.add(&val, ns);
    pc.add(&val_s, ns), pc.add(&val_t, ns), pc.add(&flag, n), pc.add(&rank, n), pc.add(&off, B + 1), pc.add(&gpos, B), pc.add(&k, B);
    pc.add(&soff, B + 1), pc.add(&temp, ns > 0 ? sort_scratch(ns) : 0);
    CHECK(pc.bytes() == o.total);
}

void grid_clusters(size_t n, size_t B, size_t dim)
{
    Old o;
    o.piece(sizeof(Grid) * B), o.piece(8 * n), o.piece(8 * n), o.piece(8 * n), o.piece(8 * n), o.piece(8 * (tiles(n) + 1));
    o.piece(8 * (B + 1)), o.piece(4 * n), o.piece(4 * n), o.piece(4 * n), o.piece(4 * n * dim), o.piece(4 * (n + 1)), o.piece(4 * 512);
    o.piece(sort_scratch(n));
    Grid *grids;
    u64 *key, *key_s, *key_t, *before, *tile;
    long long *coff;
    int32_t *perm, *perm_t, *rowptr, *longest;
    uint32_t *flag;
    float *sorted;
    char *temp;
    amp::Pieces pc;
    pc.add(&grids, B), pc.add(&key, n), pc.add(&key_s, n), pc.add(&key_t, n), pc.add(&before, n), pc.add(&tile, tiles(n) + 1);
    pc.add(&coff, B + 1), pc.add(&perm, n), pc.add(&perm_t, n), pc.add(&flag, n), pc.add(&sorted, n * dim), pc.add(&rowptr, n + 1);
    pc.add(&longest, 512), pc.add(&temp, sort_scratch(n));
    CHECK(pc.bytes() == o.total);
}

// the sampler's two stretches: before the entry count N is known (m seeds), and after
void sampler(size_t m, size_t N, size_t n_waves)
{
    Old head;
    head.piece(4 * m), head.piece(8 * m), head.piece(8 * (tiles(m) + 1)), head.piece(4 * (m + 1)), head.piece(16), head.piece(8), head.piece(4 * m);
    uint32_t *cnt;
    u64 *off, *tile, *zero;
    int32_t *brow, *flags, *seed_vm;
    amp::Pieces ph;
    ph.add(&cnt, m), ph.add(&off, m), ph.add(&tile, tiles(m) + 1), ph.add(&brow, m + 1), ph.add(&flags, 4), ph.add(&zero, 1), ph.add(&seed_vm, m);
    CHECK(ph.bytes() == head.total);
    std::vector<char> store(ph.bytes());
    ph.place(store.data());
    CHECK((char *)zero - (char *)flags == 256);                        // one memset clears the flags and the zero word behind them

    Old body;
    body.piece(4 * (m + N)), body.piece(4 * N), body.piece(4 * N), body.piece(4 * N), body.piece(4 * N), body.piece(4 * N), body.piece(4 * N);
    body.piece(4 * N), body.piece(8 * N), body.piece(8 * (tiles(N) + 1)), body.piece(sort_scratch(N)), body.piece(8 * N);
    body.piece(4 * (m + N)), body.piece(4 * m), body.piece(16 * n_waves);
    int32_t *vm, *gcol, *perm, *perm_t, *ja, *cdeg, *rdeg;
    uint32_t *key, *key_s, *key_t, *flag, *stat;
    u64 *before, *btile;
    char *temp;
    amp::Pieces pb;
    pb.add(&vm, m + N), pb.add(&gcol, N), pb.add(&key, N), pb.add(&key_s, N), pb.add(&key_t, N), pb.add(&perm, N), pb.add(&perm_t, N);
    pb.add(&flag, N), pb.add(&before, N), pb.add(&btile, tiles(N) + 1), pb.add(&temp, sort_scratch(N)), pb.add(&ja, 2 * N);
    pb.add(&cdeg, m + N), pb.add(&rdeg, m), pb.add(&stat, 4 * n_waves);
    CHECK(pb.bytes() == body.total);
}

} // namespace

int main()
{
    carve_and_write();
    contraction(1), contraction(257);
    topk(1, 0, 1), topk(300, 300, 2);
    grid_clusters(257, 2, 3);
    sampler(1, 0, 4), sampler(300, 2049, 300);
    printf("pieces: ok\n");
    return 0;
}
