// Internal to the conv launchers: the kernel families' halves of launch_conv_nt's and
// launch_conv_wgrad's switches (conv.hip). The launch templates are local to the file that holds
// their kernels (conv_v2.hip, conv_pp.hip, skinny.hip, wgrad_patch.hip), so each family exposes
// one function that launches the instantiation a plan names and decides nothing. Everything else
// calls launch_conv_nt / launch_conv_wgrad (conv.h). The kernels that take their LDS as dynamic
// shared memory are all launched through launch_lds below; what the kernel files share on the
// device side is in conv_tile.h.
#pragma once
#include "conv.h"

hipError_t launch_conv_nt_tile(int dtype, const ConvNtPlan& p, const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_nt_pp(int dtype, const ConvNtPlan& p, const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_skinny(int dtype, const ConvNtPlan& p, const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_wgrad_v2(int dtype, const ConvWgradPlan& p, const WgradArgs& a, hipStream_t s);
hipError_t launch_conv_wgrad_pp(int dtype, const ConvWgradPlan& p, const WgradArgs& a, hipStream_t s);
hipError_t launch_conv_wgrad_patch(int dtype, const ConvWgradPlan& p, const WgradArgs& a, hipStream_t s);

// Launch KERN with `lds` bytes of dynamic LDS (above the 64 KB default, so the kernel's limit is
// raised first: once per kernel instantiation and process; an instantiation always asks for the
// same bytes, the constant its launcher static_asserts against conv_select.h).
template <auto KERN, typename Args>
hipError_t launch_lds(dim3 grid, dim3 block, int lds, hipStream_t s, const Args& a) {
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    attr = true;
  }
  hipLaunchKernelGGL(KERN, grid, block, lds, s, a);
  return hipGetLastError();
}
