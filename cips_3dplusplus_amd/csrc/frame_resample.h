// Tile constants of the frame resampler (frame_resample.hip), in one place: the host's route selection, the kernels and, through
// cips3d_resample_tile, the tests read these.
#pragma once

constexpr int RS_TILE_H = 32, RS_TILE_W = 64;      // output tile of a workgroup of the fused route
constexpr int RS_THREADS = 256;
constexpr int RS_QUADS = RS_TILE_W / 4;            // a thread makes four consecutive output bytes: one dword
constexpr int RS_MAX_STAGE_ROWS = 256;             // input rows the fused route stages per tile, at the most
constexpr int RS_LDS_BYTES = 160 * 1024;           // a gfx950 workgroup's LDS: bounds the staged rows x columns
constexpr int RS_MAX_BLOCKS = 65535;               // no grid dimension above this: the kernels loop over their work items
constexpr int RS_PRECISION_BITS = 22;              // Pillow's PRECISION_BITS (32 - 8 - 2)
static_assert(RS_TILE_W % 4 == 0 && RS_THREADS % RS_QUADS == 0, "a row of the tile is a whole number of dword lanes");
