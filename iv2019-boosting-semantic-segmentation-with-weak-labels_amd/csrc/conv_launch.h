// Internal to the conv launchers: the kernel families' halves of launch_conv_nt's and
// launch_conv_wgrad's switches (conv.hip). The launch templates are local to the file that holds
// their kernels (conv_v2.hip, conv_pp.hip, skinny.hip, wgrad_patch.hip), so each family exposes
// one function that launches the instantiation a plan names and decides nothing. Everything else
// calls launch_conv_nt / launch_conv_wgrad (conv.h).
#pragma once
#include "conv.h"

hipError_t launch_conv_nt_tile(int dtype, const ConvNtPlan& p, const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_nt_pp(int dtype, const ConvNtPlan& p, const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_skinny(int dtype, const ConvNtPlan& p, const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_wgrad_v2(int dtype, const ConvWgradPlan& p, const WgradArgs& a, hipStream_t s);
hipError_t launch_conv_wgrad_pp(int dtype, const ConvWgradPlan& p, const WgradArgs& a, hipStream_t s);
hipError_t launch_conv_wgrad_patch(int dtype, const ConvWgradPlan& p, const WgradArgs& a, hipStream_t s);
