// What the stand-alone test programs of tests/cpp share: the FNV-1a digest that tests/hostbuild.py's fnv1a() restates, reading
// and summing whole vectors, and opening the input file named by argv[1]. Exit codes of the programs: 2 is usage or an unreadable
// input, 3 is a refused call, with e.what() on stderr.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static const unsigned long long kFnvBasis = 14695981039346656037ull;

// One step of FNV-1a: over bytes it is the published hash; the programs that sum 32-bit words pass those.
static inline unsigned long long fnv_step(unsigned long long s, unsigned long long v) { return (s ^ v) * 1099511628211ull; }

static inline unsigned long long fnv(const void* p, size_t bytes)
{
    const unsigned char* b = static_cast<const unsigned char*>(p);
    unsigned long long s = kFnvBasis;
    for (size_t i = 0; i < bytes; ++i) s = fnv_step(s, b[i]);
    return s;
}

template <class T>
static inline unsigned long long fnv(const std::vector<T>& v)
{
    return fnv(v.data(), v.size() * sizeof(T));
}

// The digest of the match lists: one step per 32-bit word of the records, not per byte.
template <class T>
static inline unsigned long long fnv_words(const std::vector<T>& v)
{
    static_assert(sizeof(T) % 4 == 0, "records of 32-bit words");
    unsigned long long s = kFnvBasis;
    for (size_t i = 0; i < v.size() * (sizeof(T) / 4); ++i) {
        std::uint32_t w;
        std::memcpy(&w, reinterpret_cast<const unsigned char*>(v.data()) + 4 * i, 4);
        s = fnv_step(s, w);
    }
    return s;
}

template <class T>
static inline bool read_all(std::FILE* f, std::vector<T>& v)
{
    return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

template <class T>
static inline void print_sum(const std::vector<T>& v)
{
    std::printf("%llu\n", fnv(v));
}

// argv[1] opened for reading. Null, after the usage line on stderr, with fewer than n_files arguments; null if it cannot be
// opened: exit 2.
static inline std::FILE* open_input(int argc, char** argv, const char* usage, int n_files = 1)
{
    if (argc < 1 + n_files) {
        std::fprintf(stderr, "usage: %s\n", usage);
        return nullptr;
    }
    return std::fopen(argv[1], "rb");
}
