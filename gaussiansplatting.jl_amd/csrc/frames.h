// Internal interface between the C ABI (gsr_ops.cpp) and frames.hip (compiled with -ffp-contract=off): the geometry frames —
// the exact depth percentile, the 16-bit depth map, the 8-bit normal map and the pick under a pixel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// what gsr_pick_point reads of a gsr_camera, passed by value
struct GsrPickCam {
    float R[9];  // world->camera, column-major as in the ABI
    float center[3];
    float focal[2];
    float principal[2];
};
// R_c2w of gsr_frame_normal8, column-major; use = 0: the normals stay in camera space
struct GsrRot {
    float r[9];
    int use;
};

size_t gsr_frames_scratch_size(int W, int H);
void gsr_launch_depth_scale(hipStream_t s, int W, int H, int C, const float* image, float min_alpha, double percentile,
                            void* stats_out, void* scratch);
void gsr_launch_frame_depth16(hipStream_t s, int W, int H, int C, const float* image, int expected, float min_alpha,
                              float depth_max, const float* scale_dev, int flip_rows, uint16_t* depth16_out);
void gsr_launch_frame_normal8(hipStream_t s, int W, int H, int C, const float* image, float min_alpha, const GsrRot& rot,
                              unsigned char* normal8_out);
void gsr_launch_pick_point(hipStream_t s, int W, int H, int C, const float* image, const GsrPickCam& cam, int px, int py,
                           int half_window, float* out4);
