// codestream_plan.h -- the host-only parts of the whole-file decoder that read sizes a file controls and nothing of the
// device: the container walk (ExtractCodestream, CodestreamBytes) and the order in which the single runner call of
// frame_decode.hip hands out a frame's sections (PlanTickets).  No HIP header and no context.h: codestream.hip and
// frame_decode.hip include it, and so does tests/fuzz/fuzz_codestream_plan.cc, which runs this very code under
// -fsanitize=address,undefined.
#ifndef JXLHIP_CODESTREAM_PLAN_H_
#define JXLHIP_CODESTREAM_PLAN_H_

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "../../include/jxl_hip_codestream.h"

namespace jxlhip {

// ---- container (decode.cc:1639-1672 ParseBoxHeader, 1674-2020 HandleBoxes): the codestream is the
// payload of the one jxlc box, or the concatenation of the jxlp payloads (4-byte big-endian index in
// front of each, bit 31 = last) in index order.  Out-of-order jxlp boxes are put in order.
// partial (jxlhip_decode_codestream_partial): the file may end anywhere -- a box cut short gives the payload that is there
// and ends the walk, and bytes that are the beginning of a signature are JXLHIP_ERR_NEED_MORE_INPUT.
inline int ExtractCodestream(const uint8_t* data, size_t size, std::vector<uint8_t>* storage, const uint8_t** cs,
                             size_t* cs_size, bool* container, bool partial = false) {
  static const uint8_t kSig[12] = {0, 0, 0, 0xC, 'J', 'X', 'L', ' ', 0xD, 0xA, 0x87, 0xA};
  *container = false;
  if (size >= 2 && data[0] == 0xFF && data[1] == 0x0A) {
    *cs = data;
    *cs_size = size;
    return JXLHIP_OK;
  }
  if (partial && size < 12 && (size == 0 || (size == 1 && data[0] == 0xFF) || memcmp(data, kSig, size) == 0))
    return JXLHIP_ERR_NEED_MORE_INPUT;
  if (size < 12 || memcmp(data, kSig, 12) != 0) return JXLHIP_ERR_BAD_STREAM;
  *container = true;
  struct Part {
    uint32_t index;
    const uint8_t* p;
    size_t n;
  };
  std::vector<Part> parts;
  bool have_jxlc = false, have_last = false;
  size_t pos = 0;
  bool cut = false;  // (partial) the box at hand ends behind the file
  while (pos < size && !cut) {
    if (size - pos < 8) {
      if (partial) break;
      return JXLHIP_ERR_BAD_STREAM;
    }
    uint64_t box = ((uint64_t)data[pos] << 24) | ((uint64_t)data[pos + 1] << 16) | ((uint64_t)data[pos + 2] << 8) | data[pos + 3];
    const uint8_t* type = data + pos + 4;
    size_t header = 8;
    if (box == 1) {  // 64-bit size follows
      if (size - pos < 16) {
        if (partial) break;
        return JXLHIP_ERR_BAD_STREAM;
      }
      box = 0;
      for (int i = 0; i < 8; i++) box = (box << 8) | data[pos + 8 + i];
      header = 16;
    }
    uint64_t payload;
    if (box == 0) payload = size - pos - header;  // runs to the end of the file
    else if (box < header) return JXLHIP_ERR_BAD_STREAM;
    else if (box - header > size - pos - header) {
      if (!partial) return JXLHIP_ERR_BAD_STREAM;
      payload = size - pos - header;
      cut = true;
    } else payload = box - header;
    const uint8_t* p = data + pos + header;
    if (!memcmp(type, "jxlc", 4)) {
      if (have_jxlc || !parts.empty()) return JXLHIP_ERR_BAD_STREAM;  // "there can only be one jxlc box"
      have_jxlc = true;
      parts.push_back({0u, p, (size_t)payload});
    } else if (!memcmp(type, "jxlp", 4)) {
      if (cut && payload < 4) break;
      if (have_jxlc || payload < 4) return JXLHIP_ERR_BAD_STREAM;
      const uint32_t idx = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
      if (idx & 0x80000000u) {
        if (have_last) return JXLHIP_ERR_BAD_STREAM;
        have_last = true;
      }
      parts.push_back({idx & 0x7FFFFFFFu, p + 4, (size_t)payload - 4});
    }
    // ftyp, jxll, Exif, xml, jumb, brob, jbrd ...: not pixels
    pos += header + payload;
  }
  if (parts.empty()) return partial ? JXLHIP_ERR_NEED_MORE_INPUT : JXLHIP_ERR_BAD_STREAM;
  if (parts.size() == 1 && have_jxlc) {
    *cs = parts[0].p;
    *cs_size = parts[0].n;
    return JXLHIP_OK;
  }
  std::sort(parts.begin(), parts.end(), [](const Part& a, const Part& b) { return a.index < b.index; });
  for (size_t i = 0; i < parts.size(); i++)
    if (parts[i].index != i) return JXLHIP_ERR_BAD_STREAM;  // duplicate or missing jxlp index
  size_t total = 0;
  for (const Part& q : parts) total += q.n;
  storage->resize(total);
  size_t at = 0;
  for (const Part& q : parts) {
    if (q.n) memcpy(storage->data() + at, q.p, q.n);  // (jxlp boxes without a byte between them: storage is empty, its data() null)
    at += q.n;
  }
  *cs = storage->data();
  *cs_size = total;
  return JXLHIP_OK;
}

// the codestream of a file: cs[0, n) points into the caller's bytes, or into `storage` when jxlp boxes were joined
struct CodestreamBytes {
  std::vector<uint8_t> storage;
  const uint8_t* cs = nullptr;
  size_t n = 0;
  bool container = false;
  int Open(const uint8_t* data, size_t size, bool partial = false) {
    return ExtractCodestream(data, size, &storage, &cs, &n, &container, partial);
  }
};

// ---- the ticket order of the single runner call (frame_decode.hip: PipelineJob).  dc_sizes: the bytes of the ndc DC-group
// sections; ac_sizes[pass * ng + g]: those of the AC-group sections.
// dc_order: the DC-phase units, first to last -- AC global (unit ndc: short, and every AC group waits for it), then the
// DC groups by descending bytes; ac_of_dc[d]: the AC groups under DC group d (8 x 8 of them, dec_frame.cc:318-360 /
// frame_dimensions.h), by descending bytes summed over the passes.  Equal sizes: the lower index first; a size from 2^32
// on counts as 2^32 - 1.  false: AC group *stray lies under no DC group.
inline bool PlanTickets(uint32_t ndc, uint32_t ng, uint32_t np, const size_t* dc_sizes, const size_t* ac_sizes, uint32_t xsize,
                        uint32_t xsize_blocks, uint32_t group_dim, std::vector<uint32_t>* dc_order,
                        std::vector<std::vector<uint32_t>>* ac_of_dc, uint32_t* stray) {
  std::vector<uint64_t> key(ndc);
  for (uint32_t g = 0; g < ndc; g++) key[g] = ((uint64_t)std::min<size_t>(dc_sizes[g], 0xFFFFFFFFu) << 32) | (uint32_t)~g;
  std::sort(key.begin(), key.end(), std::greater<uint64_t>());
  dc_order->assign(1, ndc);
  for (uint32_t g = 0; g < ndc; g++) dc_order->push_back(~(uint32_t)key[g]);
  const uint32_t xsg = (xsize + 255) / 256, xdg = (xsize_blocks + group_dim - 1) / group_dim;
  ac_of_dc->assign(ndc, std::vector<uint32_t>());
  std::vector<uint64_t> akey(ng);
  for (uint32_t g = 0; g < ng; g++) {
    uint64_t bytes = 0;
    for (uint32_t ps = 0; ps < np; ps++) bytes += ac_sizes[(size_t)ps * ng + g];
    akey[g] = (std::min<uint64_t>(bytes, 0xFFFFFFFFu) << 32) | (uint32_t)~g;
  }
  std::sort(akey.begin(), akey.end(), std::greater<uint64_t>());
  for (uint32_t t = 0; t < ng; t++) {
    const uint32_t g = ~(uint32_t)akey[t];
    const uint32_t d = (g / xsg / 8) * xdg + (g % xsg) / 8;
    if (d >= ndc) return *stray = g, false;
    (*ac_of_dc)[d].push_back(g);
  }
  return true;
}

}  // namespace jxlhip

#endif  // JXLHIP_CODESTREAM_PLAN_H_
