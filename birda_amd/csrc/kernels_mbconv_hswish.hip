// The fused MBConv kernel's tile configurations (mbconv_cfgs.inc, part 0 of 3) instantiated for ONE activation: ACT_HSWISH,
// every entry a second time as pass A of a squeeze-excite block (MB_WITH_SE, mbconv_kernel.hpp SE = 1: swish since round 5 --
// EfficientNet's, Perch v2's backbone -- GELU and ReLU6 since round 6; hard swish, MobileNetV3's, with its family).
#define MB_WITH_SE 1
#include "mbconv_kernel.hpp"

namespace bh {

namespace {
#define MB_A ACT_HSWISH
#define MB_PART 0
const MbCfg kTable[] = {
#include "mbconv_cfgs.inc"
};
#undef MB_PART
#undef MB_A
}  // namespace

const MbCfg *mb_table_hswish_p0(int *n) {
    if (n) *n = (int)(sizeof(kTable) / sizeof(kTable[0]));
    return kTable;
}

}  // namespace bh
