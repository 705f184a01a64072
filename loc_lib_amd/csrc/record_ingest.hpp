// loc_lib_amd/csrc/record_ingest.hpp — driver-specific point records decoded in HBM (record_ingest.hip; include/locgpu.h, "Point-record ingest").
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/locgpu.h"

struct locgpu_ctx;

namespace locgpu {

struct RecordIngestScratch;  // record_ingest.hip: staging and workspaces, grow-only on the context (locgpu_ctx::recingest)

// Frees them (called by locgpu_destroy).
void record_ingest_free(locgpu_ctx* ctx);

}  // namespace locgpu
