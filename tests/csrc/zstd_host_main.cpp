// zstd_host_main.cpp — the device Zstandard decoder (databend_amd/csrc/zstd_dev.hpp), host build
// (ZS_HOST), as a stand-alone program for -fsanitize=address,undefined (tests/test_zstd_host.py
// builds and runs it; nothing sanitised is loaded into the test's own process).
//
//   zstd_host_main <records> <results>
//
// records: u32 count, then per record u32 frame length, u64 output size, the frame bytes.  Every
// frame is copied into a heap block of exactly its length and decoded into a heap block of exactly
// the output size, so a read past the frame or a write past the output lands in the sanitizer's
// red zone.  results: one line per record, "0 <fnv-1a 64 of the output, hex>" for a frame that
// decoded, "1" for one that was rejected.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define ZS_HOST 1
#include "zstd_dev.hpp"

static std::vector<u8> slurp(const char* path) {
    std::vector<u8> out;
    FILE* f = fopen(path, "rb");
    if (!f) return out;
    static u8 buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return out;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <records> <results>\n", argv[0]);
        return 2;
    }
    const std::vector<u8> in = slurp(argv[1]);
    if (in.size() < 4) return 2;
    FILE* res = fopen(argv[2], "w");
    if (!res) return 2;
    u32 n;
    memcpy(&n, in.data(), 4);
    size_t at = 4;
    ZsTables* T = (ZsTables*)calloc(1, sizeof(ZsTables));
    ZsWork* W = (ZsWork*)calloc(1, sizeof(ZsWork));
    for (u32 c = 0; c < n; ++c) {
        if (at + 12 > in.size()) return 3;
        u32 fl;
        u64 dn;
        memcpy(&fl, in.data() + at, 4);
        memcpy(&dn, in.data() + at + 4, 8);
        at += 12;
        if (at + fl > in.size()) return 3;
        u8* frame = (u8*)malloc(fl ? fl : 1);
        u8* dst = (u8*)malloc(dn ? dn : 1);
        u8* lit = (u8*)malloc(ZS_MAX_BLOCK);
        if (fl) memcpy(frame, in.data() + at, fl);
        at += fl;
        // the tables and the ring keep what the last record left, as the LDS of a wave does
        const bool ok = zs_decode(frame, fl, dst, dn, lit, *T, *W);
        if (ok) {
            u64 h = 0xcbf29ce484222325ULL;
            for (u64 i = 0; i < dn; ++i) h = (h ^ dst[i]) * 0x100000001b3ULL;
            fprintf(res, "0 %016llx\n", (unsigned long long)h);
        } else {
            fprintf(res, "1\n");
        }
        free(lit);
        free(dst);
        free(frame);
    }
    free(W);
    free(T);
    fclose(res);
    return 0;
}
