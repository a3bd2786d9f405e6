// rsn_field_split.hip -- the split-bf16 instantiations of the field kernel (RSN_MMA_BF16X6: eval and training, RSN_MMA_BF16X3:
// eval), compiled WITHOUT -amdgpu-mfma-vgpr-form (rsn_field_kernel.h says why).
#include "rsn_field_kernel.h"

int rsn_launch_field_split(int width, bool train, rsn_mma_mode mode, long long grid, hipStream_t st, const FieldJobs& J) {
  RSN_REQUIRE(mode == RSN_MMA_BF16X6 || (mode == RSN_MMA_BF16X3 && !train), RSN_ERR_INVALID_ARGUMENT, "split launch: mode=%d train=%d",
              (int)mode, (int)train);
  return rsn_for_width(width, [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    const dim3 g((unsigned)grid), b(256);
    if (train) hipLaunchKernelGGL((rsn_field_kernel<NB, true, RSN_MMA_BF16X6>), g, b, 0, st, J);
    else if (mode == RSN_MMA_BF16X6) hipLaunchKernelGGL((rsn_field_kernel<NB, false, RSN_MMA_BF16X6>), g, b, 0, st, J);
    else hipLaunchKernelGGL((rsn_field_kernel<NB, false, RSN_MMA_BF16X3>), g, b, 0, st, J);
  });
}
