// gms_resample.h -- the library's one implementation of Pillow's 8-bit separable resampling (resize.hip), as its two entry points
// see it: gms_resize_u8 hands it the source bytes, gms_ground_truth_u8 (images.hip) the pixels it has composited.
#pragma once
#include "gms_common.h"

namespace gms {

// What a source pixel is: the channels resampled, its bytes, and whether RGBA is premultiplied as it is read.
enum class ResamplePixel {
    RGB,            // three channels in three bytes
    RGBA,           // four channels in an aligned word, premultiplied on the way in, un-premultiplied and alpha dropped on the way out
    RGB_IN_WORD,    // three channels in an aligned word whose fourth byte is never read: composited pixels
};

struct ResampleJob {
    int32_t images, h, w, oh, ow;
    const int32_t *h_bounds, *h_coeffs, *v_bounds, *v_coeffs;      // device tables of an axis that changes
    int32_t h_kmax, v_kmax;
    const uint8_t *src;             // [images,h,w] pixels of `pixel`'s kind
    ResamplePixel pixel;
    uint8_t *work;                  // [images,h,ow] four-byte pixels between the passes when both axes change, 16-byte aligned
    float *out;                     // [images,3,oh,ow]
};

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// bytes of ResampleJob::work: 0 unless both axes change
size_t resample_work_bytes(int64_t images, int64_t h, int64_t w, int64_t oh, int64_t ow);

// The checks the entry points share, on the caller's arguments (job.src is the caller's source of `channels` bytes a pixel, job.work
// is not read): positive sizes, channels 3 or 4, null pointers, the tables and kmax of an axis that changes, at most 65 535 images,
// the grid size, and a workspace of `need` bytes (0: none is used) present, 16-byte aligned and large enough.  Sets the error text,
// prefixed with `entry`, and returns GMS_ERR_INVALID_ARGUMENT or GMS_ERR_CAPACITY; GMS_OK when the call may go ahead.
int32_t check_resample_args(const char *entry, const ResampleJob &job, int32_t channels, const void *workspace, size_t workspace_bytes, size_t need);

// Launches the passes of a checked job: one per axis that changes, one copy at an unchanged size.  Returns the launches made.
int32_t resample_launch(const ResampleJob &job, hipStream_t stream);

}  // namespace gms
