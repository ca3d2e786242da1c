// modular_image.h -- a regular Modular frame (lossless files) on the host, in the stages frame_decode.hip runs: what
// modular_image.inc (part of entropy.cc) offers beside the one public entry jxlhip_modular_image_decode
// (include/jxl_hip_frame.h), which is these stages glued.  No device, no HIP header.
#ifndef JXLHIP_MODULAR_IMAGE_H_
#define JXLHIP_MODULAR_IMAGE_H_

#include <stddef.h>
#include <stdint.h>

#include "../../include/jxl_hip_frame.h"

namespace jxlhip {
extern "C" {  // (entropy.cc is one extern "C" unit: the names carry no namespace in the object file; they stay hidden)

struct ModularImage;  // one frame's state: the global tree, the global image, where the planes go

// The frame-header conditions of jxlhip_modular_image_decode: nullptr, or the case it refuses (a static string)
const char* ModularImageRefusal(const jxlhip_frame_header* fh);

// DC global of a regular Modular frame from bit *bit_pos of its first section (advanced): DequantMatrices::DecodeDC, the
// global tree and the global Modular image.  out->planes / stride_samples / sample_type / group_rct are taken from *out
// and must stay valid until ModularImageFinish has returned; *why as in jxlhip_modular_image_decode.
int ModularImageBegin(const uint8_t* data, size_t size, size_t* bit_pos, const jxlhip_frame_header* fh,
                      jxlhip_modular_image_planes* out, ModularImage** image, const char** why);
// ModularDC(dc_group) / ModularAC(group, pass = 0) from bit *bit_pos of their sections (advanced).  Thread-safe for
// different groups.
int ModularImageDcGroup(ModularImage* image, uint32_t dc_group, const uint8_t* data, size_t size, size_t* bit_pos);
int ModularImageAcGroup(ModularImage* image, uint32_t group, const uint8_t* data, size_t size, size_t* bit_pos);
// Every group is in: what the host has to undo of the global image is undone, the planes are complete, the out fields
// of the planes struct are filled.  JXLHIP_ERR_RANGE: a sample does not fit JXLHIP_MODULAR_I16 planes.
int ModularImageFinish(ModularImage* image);
void ModularImageDestroy(ModularImage* image);

}  // extern "C"
}  // namespace jxlhip
#endif
