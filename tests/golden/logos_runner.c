/*
 * tests/golden/logos_runner.c -- generator tooling for tests/golden/refdll_logos.npz (not product, not oracle).
 *
 * Runs cv::xfeatures2d::matchLOGOS (export RVA 0x7fbc0 of the reference's SfM-GMS/bin/opencv_xfeatures2d452.dll) WHOLE,
 * straight out of the DLL's machine code: the Point constructors, Logos::Logos / init, both nearest-neighbour passes, the
 * candidate loop, local support, the orientation histogram and the DMatch output are all the DLL's own code.
 *
 * The PE image is mapped section by section into executable memory and its base relocations are applied. Its imports are
 * resolved by name against a short table of this file; every other import slot points at a trap that aborts, so a call
 * this file does not know about cannot pass unnoticed. What the table supplies:
 *   - the allocator: malloc, free, calloc, _callnewh (operator new / delete of the DLL reach the CRT heap through these);
 *   - memmove, memcpy, memset;
 *   - the four elementary functions LOGOS calls through the CRT: logf, acosf, sqrtf, ceil. They are pointed at this
 *     process's libm. sqrtf and ceil are exact in every conforming libm; logf and acosf are not required to be correctly
 *     rounded, so a result here may differ in the last bit from what the Windows CRT returns. That substitution is the one
 *     residue of the fixture.
 * Nothing of the DLL is copied into the repository: only the inputs and the matches the DLL returns are kept.
 *
 * usage: logos_runner <dll> <in.bin> <out.bin> sort
 *   The neighbour ordering alone: the std::sort instance Point::nearestNeighbours calls (RVA 0x52d60, _Sort_unchecked(first,
 *   last, ideal = last - first, pred)) with its own predicate (RVA 0x53540: a.d < b.d on the float alone), on caller-given
 *   (float d, int32 index) records. This pins the tie order of equal distances.
 *   in.bin : int32 n; n x (float d, int32 index)
 *   out.bin: the n records in the order the DLL leaves them
 *
 * usage: logos_runner <dll> <in.bin> <out.bin>
 *   in.bin : int32 n1, n2; n1 + n2 28-byte cv::KeyPoint records; n1 + n2 int32 labels (nn1, then nn2)
 *   out.bin: int64 m; m x 16-byte cv::DMatch records (int32 queryIdx, trainIdx, imgIdx; float distance)
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#define RVA_MATCH_LOGOS 0x7fbc0u
#define RVA_SORT 0x52d60u
#define RVA_SORT_PRED 0x53540u

static void* __attribute__((ms_abi)) crt_malloc(size_t n) { return malloc(n ? n : 1); }
static void* __attribute__((ms_abi)) crt_calloc(size_t n, size_t s) { return calloc(n ? n : 1, s ? s : 1); }
static void __attribute__((ms_abi)) crt_free(void* p) { free(p); }
static int __attribute__((ms_abi)) crt_callnewh(size_t n) { (void)n; return 0; }
static void* __attribute__((ms_abi)) crt_memmove(void* d, const void* s, size_t n) { return memmove(d, s, n); }
static void* __attribute__((ms_abi)) crt_memcpy(void* d, const void* s, size_t n) { return memmove(d, s, n); }
static void* __attribute__((ms_abi)) crt_memset(void* d, int c, size_t n) { return memset(d, c, n); }
static float __attribute__((ms_abi)) crt_logf(float x) { return logf(x); }
static float __attribute__((ms_abi)) crt_acosf(float x) { return acosf(x); }
static float __attribute__((ms_abi)) crt_sqrtf(float x) { return sqrtf(x); }
static double __attribute__((ms_abi)) crt_ceil(double x) { return ceil(x); }
static void __attribute__((ms_abi)) trap(void)
{
    fprintf(stderr, "logos_runner: the DLL called an import this file does not provide\n");
    abort();
}

static const struct { const char* name; void* fn; } k_imports[] = {
    {"malloc", (void*)crt_malloc}, {"calloc", (void*)crt_calloc},   {"free", (void*)crt_free},
    {"_callnewh", (void*)crt_callnewh}, {"memmove", (void*)crt_memmove}, {"memcpy", (void*)crt_memcpy},
    {"memset", (void*)crt_memset}, {"logf", (void*)crt_logf},        {"acosf", (void*)crt_acosf},
    {"sqrtf", (void*)crt_sqrtf},   {"ceil", (void*)crt_ceil},
};

static uint32_t rd32(const unsigned char* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static uint16_t rd16(const unsigned char* p) { uint16_t v; memcpy(&v, p, 2); return v; }

typedef struct { void* begin; void* end; void* cap; } msvc_vector;
typedef void(__attribute__((ms_abi)) * match_logos_fn)(const msvc_vector* kp1, const msvc_vector* kp2, const msvc_vector* nn1,
                                                        const msvc_vector* nn2, msvc_vector* matches);

int main(int argc, char** argv)
{
    if (argc != 4 && !(argc == 5 && strcmp(argv[4], "sort") == 0)) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    const long fsz = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char* file = malloc((size_t)fsz);
    if (fread(file, 1, (size_t)fsz, f) != (size_t)fsz) return 3;
    fclose(f);

    const uint32_t pe = rd32(file + 0x3c);
    if (memcmp(file + pe, "PE\0\0", 4) != 0) return 4;
    const int nsec = rd16(file + pe + 6);
    const int optsz = rd16(file + pe + 20);
    const unsigned char* opt = file + pe + 24;
    if (rd16(opt) != 0x20b) return 4; /* PE32+ */
    uint64_t image_base;
    memcpy(&image_base, opt + 24, 8);
    const uint32_t size_image = rd32(opt + 56), size_headers = rd32(opt + 60);
    unsigned char* img = mmap(NULL, (size_t)size_image + 0x1000, PROT_READ | PROT_WRITE | PROT_EXEC, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (img == MAP_FAILED) return 5;
    memcpy(img, file, size_headers);
    const unsigned char* sec = opt + optsz;
    for (int i = 0; i < nsec; i++, sec += 40) {
        const uint32_t vsize = rd32(sec + 8), va = rd32(sec + 12), rsize = rd32(sec + 16), rptr = rd32(sec + 20);
        const uint32_t n = rsize < vsize ? rsize : vsize;
        if ((uint64_t)va + n > size_image || (uint64_t)rptr + n > (uint64_t)fsz) return 4;
        memcpy(img + va, file + rptr, n);
    }
    /* base relocations (data directory 5): IMAGE_REL_BASED_DIR64 entries get the load delta */
    const uint32_t reloc_rva = rd32(opt + 112 + 5 * 8), reloc_size = rd32(opt + 112 + 5 * 8 + 4);
    const uint64_t delta = (uint64_t)(uintptr_t)img - image_base;
    for (uint32_t pos = 0; pos + 8 <= reloc_size;) {
        const uint32_t page = rd32(img + reloc_rva + pos), block = rd32(img + reloc_rva + pos + 4);
        if (block < 8) return 4;
        for (uint32_t e = 8; e + 2 <= block; e += 2) {
            const uint16_t ent = rd16(img + reloc_rva + pos + e);
            if ((ent >> 12) == 10) {
                uint64_t v;
                if ((uint64_t)page + (ent & 0xfff) + 8 > size_image) return 4;
                memcpy(&v, img + page + (ent & 0xfff), 8);
                v += delta;
                memcpy(img + page + (ent & 0xfff), &v, 8);
            } else if ((ent >> 12) != 0) {
                return 4;
            }
        }
        pos += block;
    }
    /* imports (data directory 1): known names from the table above, everything else the trap */
    const uint32_t imp_rva = rd32(opt + 112 + 1 * 8);
    for (const unsigned char* d = img + imp_rva; rd32(d + 12) != 0; d += 20) {
        const uint32_t ilt = rd32(d) ? rd32(d) : rd32(d + 16), iat = rd32(d + 16);
        for (uint32_t k = 0;; k++) {
            uint64_t ent;
            memcpy(&ent, img + ilt + 8 * k, 8);
            if (ent == 0) break;
            void* fn = (void*)trap;
            if (!(ent >> 63)) {
                const char* name = (const char*)(img + (uint32_t)(ent & 0x7fffffff) + 2);
                for (size_t t = 0; t < sizeof k_imports / sizeof k_imports[0]; t++)
                    if (strcmp(name, k_imports[t].name) == 0) fn = k_imports[t].fn;
            }
            memcpy(img + iat + 8 * k, &fn, 8);
        }
    }

    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) return 6;
    if (argc == 5) {
        typedef void(__attribute__((ms_abi)) * sort_fn)(void* first, void* last, int64_t ideal, void* pred);
        int32_t n;
        if (fread(&n, 4, 1, in) != 1 || n < 0) return 6;
        unsigned char* rec = malloc(8 * (size_t)n + 8);
        if (fread(rec, 8, (size_t)n, in) != (size_t)n) return 6;
        ((sort_fn)(img + RVA_SORT))(rec, rec + 8 * (size_t)n, n, img + RVA_SORT_PRED);
        if (fwrite(rec, 8, (size_t)n, out) != (size_t)n) return 7;
        fclose(out);
        return 0;
    }
    int32_t hdr[2];
    if (fread(hdr, 4, 2, in) != 2 || hdr[0] < 0 || hdr[1] < 0) return 6;
    const size_t n1 = (size_t)hdr[0], n2 = (size_t)hdr[1];
    unsigned char* kp = malloc(28 * (n1 + n2) + 1);
    int32_t* nn = malloc(4 * (n1 + n2) + 4);
    if (fread(kp, 28, n1 + n2, in) != n1 + n2 || fread(nn, 4, n1 + n2, in) != n1 + n2) return 6;
    fclose(in);
    msvc_vector v_kp1 = {kp, kp + 28 * n1, kp + 28 * n1};
    msvc_vector v_kp2 = {kp + 28 * n1, kp + 28 * (n1 + n2), kp + 28 * (n1 + n2)};
    msvc_vector v_nn1 = {nn, nn + n1, nn + n1};
    msvc_vector v_nn2 = {nn + n1, nn + n1 + n2, nn + n1 + n2};
    msvc_vector v_out = {NULL, NULL, NULL};
    ((match_logos_fn)(img + RVA_MATCH_LOGOS))(&v_kp1, &v_kp2, &v_nn1, &v_nn2, &v_out);
    const int64_t m = (int64_t)(((unsigned char*)v_out.end - (unsigned char*)v_out.begin) / 16);
    if (fwrite(&m, 8, 1, out) != 1 || (m && fwrite(v_out.begin, 16, (size_t)m, out) != (size_t)m)) return 7;
    fclose(out);
    return 0;
}
