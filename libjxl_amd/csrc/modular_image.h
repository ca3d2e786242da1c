// modular_image.h -- a regular Modular frame (lossless files) on the host, in the stages frame_decode.hip runs: what
// modular_image.inc (part of entropy.cc) offers beside the public entries jxlhip_modular_image_decode[_channels]
// (include/jxl_hip_frame.h), which are these stages glued.  No device, no HIP header.
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
// ... of jxlhip_modular_image_decode_channels: the same but for the image's extra channels -- up to four, none
// sub-sampled, every blend mode of this one full-size frame kReplace
const char* ModularImageChannelsRefusal(const jxlhip_frame_header* fh);

// DC global of a regular Modular frame from bit *bit_pos of its first section (advanced): DequantMatrices::DecodeDC, the
// global tree and the global Modular image of out->num_color + out->num_extra channels.  The in fields of *out are read
// and must stay valid until ModularImageFinish has returned; *why as in jxlhip_modular_image_decode_channels.
int ModularImageBegin(const uint8_t* data, size_t size, size_t* bit_pos, const jxlhip_frame_header* fh,
                      jxlhip_modular_image_channels* out, ModularImage** image, const char** why);
// ModularDC(dc_group) / ModularAC(group, pass = 0) from bit *bit_pos of their sections (advanced).  Thread-safe for
// different groups.
int ModularImageDcGroup(ModularImage* image, uint32_t dc_group, const uint8_t* data, size_t size, size_t* bit_pos);
int ModularImageAcGroup(ModularImage* image, uint32_t group, const uint8_t* data, size_t size, size_t* bit_pos);
// Every group is in: what the host has to undo of the global image is undone, the planes are complete, the out fields
// of the struct are filled.  JXLHIP_ERR_RANGE: a sample of any plane does not fit JXLHIP_MODULAR_I16 planes.
int ModularImageFinish(ModularImage* image);
void ModularImageDestroy(ModularImage* image);

}  // extern "C"
}  // namespace jxlhip
#endif
