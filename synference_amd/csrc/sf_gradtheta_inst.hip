// sf_gradtheta_inst.hip -- one translation unit per SF_HT: instantiates the theta-gradient kernels.
#include "sf_gradtheta_kernels.h"

#ifndef SF_HT
#error "compile with -DSF_HT=1..4"
#endif
#define SF_CAT_(a, b) a##b
#define SF_CAT(a, b) SF_CAT_(a, b)

// n_tiles workgroups of one wave: tile a.tile0 + i each
hipError_t SF_CAT(sf_launch_maf_gradtheta_h, SF_HT)(const SfDev& m, const SfGradThetaArgs& a, long n_tiles, hipStream_t st) {
  if (m.D <= 8) hipLaunchKernelGGL((k_maf_gradtheta<SF_HT, 8>), dim3((unsigned)n_tiles), dim3(64), 0, st, m, a);
  else hipLaunchKernelGGL((k_maf_gradtheta<SF_HT, SF_DMAX>), dim3((unsigned)n_tiles), dim3(64), 0, st, m, a);
  return hipGetLastError();
}

hipError_t SF_CAT(sf_launch_nsf_gradtheta_h, SF_HT)(const SfDev& m, const SfGradThetaArgs& a, long n_tiles, hipStream_t st) {
  switch (m.PT) {
    case 2: hipLaunchKernelGGL((k_nsf_gradtheta<SF_HT, 2>), dim3((unsigned)n_tiles), dim3(64), 0, st, m, a); break;
    case 3: hipLaunchKernelGGL((k_nsf_gradtheta<SF_HT, 3>), dim3((unsigned)n_tiles), dim3(64), 0, st, m, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
