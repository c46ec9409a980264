// opticalflow.h -- the optical-flow producer kernels' launchers (k_opticalflow.hip); their argument blocks are in opticalflow_args.h
//
// The producer is two stages.  PER IMAGE: level 0 of its pyramid (u8 gray, or 8-bit colour through OpenCV's fixed-point gray
// conversion, -> float) and the levels below it by 2 x 2 means.  PER PAIR: the Lucas-Kanade levels, coarse to fine, over the
// pyramids of the previous and the current image, and the CV_16SC2 quantisation where that is the product.  An image that is
// the `cur` of one pair and the `prev` of the next (a camera stream) has its pyramid built once.  A launch serves a chunk of at
// most kOfChunk images / pairs whose pointers travel in the kernel arguments: no pointer table in memory, nothing to copy or to
// wait for before a launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "opticalflow_args.h"

namespace roft {

void launch_of_pyramids(const OfGeom& g, const OfImages& im, hipStream_t s);
void launch_of_pairs(const OfGeom& g, const OfPairs& pr, hipStream_t s);   // (quantises when out_s16[0] is set: a chunk has one product)
// behind launch_of_pairs of a checked chunk, on the same stream: one launch, pairs in blockIdx.y
void launch_of_check(const OfGeom& g, const OfCheck& ck, hipStream_t s);
// 8-bit colour -> 8-bit gray, any W x H (the stand-alone operator)
void launch_image_to_gray(const uint8_t* src, int type, size_t npix, uint8_t* dst, hipStream_t s);

}  // namespace roft
