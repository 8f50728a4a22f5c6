// block_layout.h -- where the regions of one device block start.
//
// The one-shot host entry points of the capi_*.cpp (gms_bf_match_select, gms_stereo_bm, gms_portrait, ...) keep everything a call needs --
// inputs, tables, workspace, outputs -- in ONE device allocation. This is the arithmetic of that block, and nothing else: no HIP
// header, so that a host compiler builds it alone (tests/cpp/block_layout_check.cpp does).
#pragma once

#include <cstddef>

namespace gms {

// Hands out consecutive regions of one block, in call order. Every region starts on a kAlign boundary and is at least
// bytes + slack long; an empty region costs nothing (it shares its offset with the next one).
class BlockLayout {
public:
    static constexpr size_t kAlign = 256;

    // the offset of a new region of `bytes` bytes, with `slack` spare bytes behind it
    size_t add(size_t bytes, size_t slack = 0)
    {
        const size_t at = end_;
        end_ = (at + bytes + slack + kAlign - 1) / kAlign * kAlign;
        return at;
    }
    // the size of the block that holds every region handed out so far
    size_t total() const { return end_; }

private:
    size_t end_ = 0;
};

}  // namespace gms
