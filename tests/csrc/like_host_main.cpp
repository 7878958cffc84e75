// like_host_main.cpp — the LIKE matchers of databend_amd/csrc/like.hpp, host build (LIKE_HOST), as a
// stand-alone program for -fsanitize=address,undefined (tests/test_like_ref.py builds and runs it).
//
//   like_host_main <cases> <results>
//
// cases: u32 count, then per case u16 haystack length, u16 pattern length, the haystack bytes, the
// pattern bytes.  Every haystack and every pattern is copied into a heap block of exactly its
// length before the matcher sees it, so a read past either end (in the backtracking, a segment
// search or a suffix compare) lands in the sanitizer's red zone.  results: two characters per case,
// the pattern's class digit and '0' / '1' for the match ('x' where the pattern is beyond the caps).
#define LIKE_HOST
#include "like.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static std::vector<u8> slurp(const char* path) {
    std::vector<u8> out;
    FILE* f = fopen(path, "rb");
    if (!f) return out;
    u8 buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return out;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]);
        return 2;
    }
    const std::vector<u8> in = slurp(argv[1]);
    if (in.size() < 4) return 2;
    u32 n;
    memcpy(&n, in.data(), 4);
    size_t at = 4;
    std::vector<char> out;
    out.reserve(2 * (size_t)n);
    for (u32 c = 0; c < n; ++c) {
        if (at + 4 > in.size()) return 3;
        uint16_t hl, pl;
        memcpy(&hl, in.data() + at, 2);
        memcpy(&pl, in.data() + at + 2, 2);
        at += 4;
        if (at + hl + pl > in.size()) return 3;
        u8* h = (u8*)malloc(hl);
        u8* p = (u8*)malloc(pl);
        if (hl) memcpy(h, in.data() + at, hl);
        if (pl) memcpy(p, in.data() + at + hl, pl);
        at += (size_t)hl + pl;
        LikeDesc L;
        if (pl > DBG_LIKE_MAX_PATTERN || !like_classify(p, pl, L)) {
            out.push_back('x');
            out.push_back('x');
        } else {
            out.push_back((char)('0' + L.kind));
            out.push_back(like_match(L, (const u8*)h, (u64)hl, (const u8*)p) ? '1' : '0');
        }
        free(h);
        free(p);
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.data(), 1, out.size(), f);
    fclose(f);
    return 0;
}
