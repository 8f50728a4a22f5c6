// tests/test_speckle_ref.py: the speckle filter's host statement (speckle_core.h, the header the kernels compile) built by a host
// compiler alone. Usage: speckle_host IN OUT. IN: int32 width, height, new_val, max_speckle_size, max_diff, then the int16 map;
// OUT: int32 removed, then the filtered map. Exit 2: arguments refused by spk::args_ok; 1: a file that cannot be read or written.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "speckle_core.h"

int main(int argc, char** argv)
{
    if (argc != 3) return 1;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t head[5];
    if (std::fread(head, 4, 5, f) != 5) {
        std::fclose(f);
        return 1;
    }
    if (!spk::args_ok(head[0], head[1], 1, head[2], head[3], head[4])) {
        std::fclose(f);
        return 2;
    }
    const size_t px = (size_t)head[0] * (size_t)head[1];
    std::vector<int16_t> img(px);
    const size_t got = std::fread(img.data(), 2, px, f);
    std::fclose(f);
    if (got != px) return 1;
    const int32_t removed = spk::filter_host(img.data(), head[0], head[1], head[2], head[3], head[4]);
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 1;
    const bool ok = std::fwrite(&removed, 4, 1, o) == 1 && std::fwrite(img.data(), 2, px, o) == px;
    return std::fclose(o) == 0 && ok ? 0 : 1;
}
