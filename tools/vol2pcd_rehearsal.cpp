// vol2pcd_rehearsal.cpp -- the work-buffer layout of csrc/vol2pcd.hip on the CPU: ScratchLayout's pointers against the
// places written out by hand below (the order and sizes of the buffers, each on a 256-byte boundary), its two aliases,
// every buffer filled to its full length inside one malloc of `bytes`.  Host code only: no kernel runs, no device.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//       -I plant-3d-vision_amd/csrc tools/vol2pcd_rehearsal.cpp -o build/vol2pcd_rehearsal && build/vol2pcd_rehearsal
#include "vol2pcd.hip"

static int g_fail = 0;

static void expect(bool ok, const char *what, const int64_t *d) {
    if (ok) return;
    printf("%lld x %lld x %lld: %s\n", (long long)d[0], (long long)d[1], (long long)d[2], what);
    ++g_fail;
}

static void run(int64_t planes, int64_t ny, int64_t nz) {
    const int64_t d[3] = {planes, ny, nz};
    const size_t n = (size_t)(planes * ny * nz);
    const size_t nbxy = (size_t)(((planes + 7) / 8) * ((ny + 7) / 8)), nb = nbxy * (size_t)((nz + 7) / 8);
    const size_t nchunks = (size_t)(planes * ny * ((nz + 1023) / 1024));
    const size_t sizes[16] = {n, nb, nb, nb * 4, nb * 4, nbxy * 4, 64, (size_t)planes * 8, nchunks * 4, nchunks * 8,
                              n * 8, n * 8, n * 8, n * 8, n * 8, n * 8};
    size_t at[17] = {0};
    for (int k = 0; k < 16; ++k) at[k + 1] = at[k] + ((sizes[k] + 255) & ~(size_t)255);

    const ScratchLayout plan(planes, ny, nz);
    expect(plan.bytes == at[16], "bytes", d);
    expect(!plan.occ && !plan.total && !plan.g1 && !plan.gz, "pointers without a base", d);

    char *base = static_cast<char *>(malloc(plan.bytes));
    const ScratchLayout lay(planes, ny, nz, base);
    expect(lay.bytes == plan.bytes, "bytes with a base", d);
    const void *got[16] = {lay.occ, lay.cls, lay.act, lay.list_act, lay.list_halo, lay.list_cols, lay.list_n, lay.plane_sum,
                           lay.counts, lay.offsets, lay.sd, lay.ga, lay.gb, lay.gx, lay.gy, lay.gz};
    for (int k = 0; k < 16; ++k) expect(got[k] == base + at[k], "a buffer's place", d);
    expect((char *)lay.total == (char *)lay.list_n + 16, "the total behind the three lengths", d);
    expect((void *)lay.g0 == (void *)lay.ga && lay.g1 == lay.g0 + n, "the EDT buffers in ga", d);
    // every buffer at its full length (ASan: inside the allocation; the values: no buffer reaches into the next)
    for (int k = 15; k >= 0; --k) memset(const_cast<void *>(got[k]), k + 1, sizes[k]);
    for (int k = 0; k < 16; ++k)
        if (sizes[k]) expect(((const char *)got[k])[0] == k + 1 && ((const char *)got[k])[sizes[k] - 1] == k + 1, "a buffer overwritten", d);
    memset(lay.g0, 0, n * 4);
    memset(lay.g1, 0, n * 4);
    *lay.total = 0;
    lay.list_n[2] = 0;
    free(base);
}

int main() {
    const int64_t dims[][3] = {{2, 2, 2}, {9, 8, 12}, {7, 5, 9}, {70, 7, 9}, {52, 7, 9}, {64, 33, 17}, {20, 33, 1030}, {8, 8, 2100}, {3, 257, 1024}};
    for (const auto &d : dims) run(d[0], d[1], d[2]);
    printf(g_fail ? "FAILED: %d\n" : "ok: %d\n", g_fail ? g_fail : (int)(sizeof dims / sizeof dims[0]));
    return g_fail ? 1 : 0;
}
