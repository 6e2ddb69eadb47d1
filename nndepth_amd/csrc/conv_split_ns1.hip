// conv_split_kernel instantiations for arithmetic 1 ("fp16": ONE range-scaled fp16 piece, 1 product on v_mfma_f32_32x32x16_f16 —
// 11 significand bits per operand, split_arith.h).
#include "conv_split_kernel.h"

namespace nnd {
template int launch_split_ns<1>(const ConvArgs&, const SplitCfg&, int, int, hipStream_t);
#ifdef NND_DBG_STAMPS
extern "C" int nnd_debug_read_split_stamps_ns1(unsigned long long* host, int n) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_split_stamps), sizeof(unsigned long long) * n) == hipSuccess ? 0 : -1;
}
#endif
}  // namespace nnd
