// ivf_probe.h -- the probe of a clustered index, shared between the translation units whose lists have half-precision
// centroids (dense_ivf.hip, which defines it, and dense_ivfpq.hip).  Hidden visibility: not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One pass of nq <= 1024 queries f32[nq][dim_pad] (16-byte aligned) against `nlist` centroids packed as a half corpus of
// `type` (srx_half_type): cscores f32[nq][ldc] receives EVERY centroid's score (ldc = ceil(nlist / 32) * 32; the bits of
// srx_dense_score_docs_half), probe_list / probe_score [nq][nprobe] the min(nprobe, nlist) best by (score descending, list
// ascending), padded with -1 / +0.0f.  The caller has checked the arguments and set the device.
int srx_ivf_probe_pass(const void *centroids, int nlist, int type, int dim_pad, const float *queries, int nq, int nprobe, int32_t *probe_list,
                       float *probe_score, float *cscores, int64_t ldc, hipStream_t stream);
