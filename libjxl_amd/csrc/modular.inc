// modular.inc -- the slice of Modular mode that VarDCT frames need (SURVEY.md section 8, row f4):
// the global MA tree of the DC-global section, and the DC groups (quantized DC image, strategy
// map, quant field, EPF sharpness, colour-correlation maps).  Textually included by entropy.cc
// (it shares its bit reader, entropy code and field coders).  Host code, written from the format
// as the libjxl tree implements it (lib/jxl/):
//   DecodeTree / ValidateTree                      modular/encoding/dec_ma.cc:37-179
//   GroupHeader, weighted::Header                   modular/encoding/encoding.h:32-55,
//                                                   modular/encoding/context_predict.h:34-63
//   ModularDecode (channel loop, tree choice)       modular/encoding/encoding.cc:553-680
//   the per-pixel properties and predictors         modular/encoding/context_predict.h:384-545
//   the self-correcting ("weighted") predictor      modular/encoding/context_predict.h:65-196
//   DecodeGlobalInfo / DecodeVarDCTDC / DecodeAcMetadata    dec_modular.cc:207-316,427-562
//   extra channels (alpha, ...) of a VarDCT frame: the global Modular image and its per-AC-group streams
//                                                   dec_modular.cc:207-316,330-425,686-737,739-790
// ONE decode loop (the reference's "slowest track"); its fast tracks are special cases of it
//   palettes without deltas                         modular/transform/palette.cc:29-100,177-200, palette.h:53-122
//   squeeze of the frame's global image             modular/transform/squeeze.cc, dec_frame.cc:330-337 (ModularDC)
// with the same results.  Outside this slice and reported as JXLHIP_ERR_UNSUPPORTED: every transform but the
// palettes without deltas libjxl's encoder applies to extra channels with few values (one channel, or one table over
// several channels with the implicit colour-cube entries) and the squeeze `cjxl -p` puts on the global image behind
// them (RCT, delta palettes, a squeeze inside a group stream or in front of another transform), LZ77 with the 2-D
// special distances, and chroma subsampling (the back-end is 4:4:4).
// The streams of a regular Modular frame (a lossless file: modular_image.inc, ModularStreamOptions below) also carry
//   the reversible colour transforms, all 42         modular/transform/transform.cc:36-90, rct.cc:29-148
// which are read, and undone here (UndoRct) or left for the device, and LZ77.

struct jxlhip_modular_tree;

namespace {

struct MaNode {
  int32_t property;  // -1: leaf
  int32_t splitval;
  uint32_t lchild, rchild;  // property > splitval goes left
  uint32_t leaf_id, predictor, multiplier;
  int64_t offset;
};

struct WpHeader {
  int32_t p1C = 16, p2C = 10, p3Ca = 7, p3Cb = 7, p3Cc = 7, p3Cd = 0, p3Ce = 0;
  uint32_t w[4] = {0xd, 0xc, 0xc, 0xc};
};

}  // namespace

namespace {
struct ModularFull;  // the frame's extra-channel image (below)
}
struct jxlhip_modular_tree {
  std::vector<MaNode> nodes;
  EntropyCode code;
  std::shared_ptr<ModularFull> full;
};

namespace {

// the hot channel loops below exist twice, for the baseline x86-64 and for x86-64-v3 (clang's function multi-versioning;
// hipcc also walks this host file once for the device, where it means nothing, and the sanitizer harnesses build with GCC)
#if defined(__clang__) && defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define JXLHIP_X86_64_V3_CLONE __attribute__((target_clones("default", "arch=x86-64-v3")))
#else
#define JXLHIP_X86_64_V3_CLONE
#endif

constexpr uint32_t kNumModularPredictors = 14, kNumNonrefProperties = 16, kWpProperty = 15;

inline int64_t UnpackSigned64(uint64_t v) { return (int64_t)(v >> 1) ^ -(int64_t)(v & 1); }

// dec_ma.cc:37-104: every split must cut the range its property can still take on the path to it
bool ValidateMaTree(const std::vector<MaNode>& tree) {
  int num_properties = 0;
  for (const MaNode& n : tree) num_properties = std::max(num_properties, n.property + 1);
  std::vector<std::pair<int32_t, int32_t>> range(num_properties, {INT32_MIN, INT32_MAX});
  struct Item {
    uint32_t node;
    int32_t l, u;
    int action;
  };
  std::vector<Item> stack;
  stack.push_back({0, 0, 0, 0});
  while (!stack.empty()) {
    if (stack.size() >= 2048) return false;  // too tall
    Item& it = stack.back();
    const MaNode& n = tree[it.node];
    if (it.action == 0) {
      if (n.property == -1) {
        stack.pop_back();
        continue;
      }
      const int32_t l = range[n.property].first, u = range[n.property].second;
      if (l > n.splitval || u <= n.splitval) return false;
      it.l = l;
      it.u = u;
      it.action = 1;
      range[n.property].first = n.splitval + 1;
      const uint32_t child = n.lchild;
      stack.push_back({child, 0, 0, 0});
    } else if (it.action == 1) {
      it.action = 2;
      range[n.property].first = it.l;
      range[n.property].second = n.splitval;
      const uint32_t child = n.rchild;
      stack.push_back({child, 0, 0, 0});
    } else {
      range[n.property].second = it.u;
      stack.pop_back();
    }
  }
  return true;
}

// DecodeTree (dec_ma.cc:106-179) + the DecodeHistograms for its leaves that always follows
int DecodeMaTree(BitReader* br, size_t size_limit, jxlhip_modular_tree* t) {
  enum { kSplitVal = 0, kProperty = 1, kPredictor = 2, kOffset = 3, kMulLog = 4, kMulBits = 5, kNumTreeContexts = 6 };
  EntropyCode tc;
  int rc = DecodeEntropyCode(br, kNumTreeContexts, &tc, false, 0);
  if (rc) return rc;
  SymbolReader reader(&tc, br);
  if (!reader.Ok()) return JXLHIP_ERR_OUT_OF_MEMORY;
  const uint8_t* cm = tc.context_map.data();
  size_limit = std::min<size_t>(size_limit, 1u << 22);
  std::vector<MaNode>& tree = t->nodes;
  tree.clear();
  size_t to_decode = 1;
  uint32_t leaf_id = 0;
  while (to_decode > 0) {
    if (!br->Healthy() || tree.size() > size_limit) return kBad;
    to_decode--;
    const uint32_t prop1 = reader.ReadHybridUint(cm[kProperty], br);
    if (prop1 > 256) return kBad;
    MaNode n = {};
    n.property = (int32_t)prop1 - 1;
    if (n.property == -1) {
      n.predictor = reader.ReadHybridUint(cm[kPredictor], br);
      if (n.predictor >= kNumModularPredictors) return kBad;
      n.offset = UnpackSigned64(reader.ReadHybridUint(cm[kOffset], br));
      const uint32_t mul_log = reader.ReadHybridUint(cm[kMulLog], br);
      if (mul_log >= 31) return kBad;
      const uint32_t mul_bits = reader.ReadHybridUint(cm[kMulBits], br);
      if (mul_bits >= (1u << (31u - mul_log)) - 1u) return kBad;
      n.multiplier = (mul_bits + 1u) << mul_log;
      n.leaf_id = leaf_id++;
    } else {
      n.splitval = (int32_t)UnpackSigned64(reader.ReadHybridUint(cm[kSplitVal], br));
      n.lchild = (uint32_t)(tree.size() + to_decode + 1);
      n.rchild = (uint32_t)(tree.size() + to_decode + 2);
      n.multiplier = 1;
      to_decode += 2;
    }
    tree.push_back(n);
  }
  if (reader.Corrupt() || !reader.FinalStateOk() || !br->Healthy()) return kBad;
  if (!ValidateMaTree(tree)) return kBad;
  return DecodeEntropyCode(br, (tree.size() + 1) / 2, &t->code, false, 0);
}

// Transform (modular/transform/transform.h:60-137, transform.cc:36-90): the one kind taken here is the palette of a
// SINGLE channel without delta entries ("channel compaction": what libjxl's encoder applies per group to an extra
// channel that uses few of its values, enc_modular.cc:400-440,1427-1440)
struct ModularPalette {
  uint32_t begin_c = 0, num_c = 1, nb_colors = 0;
  // the same list also carries the RCTs of a regular Modular frame's streams (ModularStreamOptions::rct), in coded order:
  // rct: channels begin_c .. begin_c + 2 went through reversible colour transform rct_type (0 .. 41, rct.cc:97-148)
  bool rct = false;
  uint32_t rct_type = 0;
};
// What the streams of a regular Modular frame (jxlhip_modular_image_decode) may carry beyond the slice above, and what
// becomes of their RCTs
constexpr uint32_t kMaxDeviceRcts = 2;  // JXLHIP_MODULAR_MAX_RCTS
struct ModularStreamOptions {
  bool rct = false;         // RCTs are read (otherwise JXLHIP_ERR_UNSUPPORTED, as ever)
  bool lz77 = false;        // as ModularDecodeImage's allow_lz77
  bool leave_rcts = false;  // a transform list that is nothing but 1 .. kMaxDeviceRcts RCTs over the three colour
                            // channels (begin_c == 0) of an image of `channels` channels is NOT undone: `program` says
                            // which they were
  uint32_t channels = 3;    // ... three colour channels and the image's extra channels behind them
  // out
  bool transforms = false;  // the stream's header listed transforms
  bool left = false;        // ... and they were left (leave_rcts)
  uint16_t program = 0;     // left: the first-listed type | the second-listed type << 8 (type 0 is the identity)
};
struct SqueezeStep {  // SqueezeParams (squeeze_params.cc:15-24)
  bool horizontal = false, in_place = false;
  uint32_t begin_c = 0, num_c = 0;
};
struct ModularSqueeze {
  bool present = false;
  std::vector<SqueezeStep> steps;  // as coded; empty = the default sequence for the image's shape
};

// GroupHeader (encoding.h:37-49) with its weighted::Header and transforms; a header that announces any other
// transform is refused (before a pixel is decoded).  squeeze == NULL: a squeeze is refused too; otherwise ONE squeeze
// is taken when it is the last transform (behind the palettes: the order libjxl's encoder writes, enc_modular.cc)
int ReadModularGroupHeader(BitReader* br, bool* use_global_tree, WpHeader* wp, std::vector<ModularPalette>* palettes,
                           ModularSqueeze* squeeze = nullptr, bool allow_rct = false) {
  FieldReader r(br);
  *use_global_tree = r.Bool();
  *wp = WpHeader();
  if (!r.Bool()) {
    wp->p1C = (int32_t)r.Bits(5);
    wp->p2C = (int32_t)r.Bits(5);
    wp->p3Ca = (int32_t)r.Bits(5);
    wp->p3Cb = (int32_t)r.Bits(5);
    wp->p3Cc = (int32_t)r.Bits(5);
    wp->p3Cd = (int32_t)r.Bits(5);
    wp->p3Ce = (int32_t)r.Bits(5);
    for (uint32_t& w : wp->w) w = r.Bits(4);
  }
  static const U32Dist kNumTransforms = {{0, 0, 4, 8}, {0, 1, 2, 18}};
  const uint32_t num_transforms = r.U32(kNumTransforms);
  if (!br->Healthy()) return kBad;
  palettes->clear();
  for (uint32_t i = 0; i < num_transforms; i++) {
    static const U32Dist kId = {{0, 0, 0, 0}, {0, 1, 2, 3}};
    const uint32_t id = r.U32(kId);
    if (!br->Healthy() || id == 3) return kBad;
    if (squeeze && squeeze->present) return JXLHIP_ERR_UNSUPPORTED;  // a transform behind the squeeze
    if (id == 2 && squeeze) {  // transform.cc:78-87
      static const U32Dist kNumSqueezes = {{0, 4, 6, 8}, {0, 1, 9, 41}};
      const uint32_t n = r.U32(kNumSqueezes);
      squeeze->present = true;
      squeeze->steps.resize(n);
      for (SqueezeStep& q : squeeze->steps) {
        q.horizontal = r.Bool();
        q.in_place = r.Bool();
        static const U32Dist kBeginC = {{3, 6, 10, 13}, {0, 8, 72, 1096}};
        q.begin_c = r.U32(kBeginC);
        static const U32Dist kNumC = {{0, 0, 0, 4}, {1, 2, 3, 4}};
        q.num_c = r.U32(kNumC);
      }
      if (!br->Healthy()) return kBad;
      continue;
    }
    if (id == 0 && allow_rct) {  // transform.cc:47-60
      ModularPalette t;
      static const U32Dist kBeginC = {{3, 6, 10, 13}, {0, 8, 72, 1096}};
      t.begin_c = r.U32(kBeginC);
      static const U32Dist kRctType = {{0, 2, 4, 6}, {6, 0, 2, 10}};
      t.rct_type = r.U32(kRctType);
      if (!br->Healthy() || t.rct_type >= 42) return kBad;
      t.rct = true;
      t.num_c = 3;
      palettes->push_back(t);
      continue;
    }
    if (id != 1) return JXLHIP_ERR_UNSUPPORTED;  // RCT; squeeze of a group stream
    ModularPalette t;
    static const U32Dist kBeginC = {{3, 6, 10, 13}, {0, 8, 72, 1096}};
    t.begin_c = r.U32(kBeginC);
    static const U32Dist kNumC = {{0, 0, 0, 13}, {1, 3, 4, 1}};
    const uint32_t num_c = r.U32(kNumC);
    static const U32Dist kColors = {{8, 10, 12, 16}, {0, 256, 1280, 5376}};
    t.nb_colors = r.U32(kColors);
    static const U32Dist kDeltas = {{0, 8, 10, 16}, {0, 1, 257, 1281}};
    const uint32_t nb_deltas = r.U32(kDeltas);
    const uint32_t predictor = r.Bits(4);
    if (!br->Healthy() || predictor >= kNumModularPredictors) return kBad;
    if (nb_deltas != 0 || predictor != 0) return JXLHIP_ERR_UNSUPPORTED;  // delta palettes (lossy)
    t.num_c = num_c;
    palettes->push_back(t);
  }
  return kOk;
}

struct ModularChannel {
  uint32_t w = 0, h = 0;
  int32_t hshift = 0, vshift = 0;
  std::vector<int32_t> px;
  void Resize(uint32_t ww, uint32_t hh) {
    w = ww;
    h = hh;
    px.assign((size_t)w * h, 0);
  }
  void Shape(uint32_t ww, uint32_t hh) {  // dimensions only: the samples are allocated by whoever needs them
    w = ww;
    h = hh;
    px.clear();
  }
  int32_t* Row(uint32_t y) { return px.data() + (size_t)y * w; }
  const int32_t* Row(uint32_t y) const { return px.data() + (size_t)y * w; }
};

// the self-correcting predictor's state (context_predict.h:65-196): four sub-predictors whose
// weights follow their recent errors; all arithmetic on values carrying 3 extra bits
struct WpState {
  static constexpr int kExtra = 3;
  static constexpr int64_t kRound = ((1 << kExtra) >> 1) - 1;
  const WpHeader& hd;
  size_t xsize;
  int64_t prediction[4] = {}, pred = 0;
  // per column and row parity: the four sub-predictors' errors and the true error, side by side (one cache line
  // serves the N / NE / NW look-ups of a pixel)
  struct alignas(32) Col {
    uint32_t pe[4];
    int32_t err;
  };
  std::vector<Col> st;  // [2][xsize + 2]
  uint32_t divlookup[64];
  WpState(const WpHeader& h, size_t w) : hd(h), xsize(w) {
    st.assign((w + 2) * 2, Col{{0, 0, 0, 0}, 0});
    for (uint32_t i = 0; i < 64; i++) divlookup[i] = (1u << 24) / (i + 1);
  }
  static inline uint32_t ErrorWeightOf(uint64_t x, uint32_t maxweight, const uint32_t* divlookup) {
    int shift = (int)(63 - __builtin_clzll(x + 1)) - 5;
    if (shift < 0) shift = 0;
    return 4 + ((maxweight * divlookup[x >> shift]) >> shift);
  }
  inline uint32_t ErrorWeight(uint64_t x, uint32_t maxweight) const { return ErrorWeightOf(x, maxweight, divlookup); }
  inline int64_t Predict(size_t x, size_t y, int64_t N, int64_t W, int64_t NE, int64_t NW, int64_t NN, int32_t* max_error) {
    const size_t cur = (y & 1) ? 0 : xsize + 2, prev = (y & 1) ? xsize + 2 : 0;
    const Col* cN = &st[prev + x];
    const Col* cNE = x < xsize - 1 ? cN + 1 : cN;
    const Col* cNW = x > 0 ? cN - 1 : cN;
    uint32_t w[4];
    for (int i = 0; i < 4; i++) w[i] = ErrorWeight(cN->pe[i] + cNE->pe[i] + cNW->pe[i] /* 32-bit sum */, hd.w[i]);
    N *= 8, W *= 8, NE *= 8, NW *= 8, NN *= 8;
    const int64_t teW = x == 0 ? 0 : st[cur + x - 1].err, teN = cN->err, teNW = cNW->err, teNE = cNE->err;
    const int64_t sumWN = teN + teW;
    int64_t p = teW;
    if (std::abs(teN) > std::abs(p)) p = teN;
    if (std::abs(teNW) > std::abs(p)) p = teNW;
    if (std::abs(teNE) > std::abs(p)) p = teNE;
    *max_error = (int32_t)p;
    prediction[0] = W + NE - N;
    prediction[1] = N - (((sumWN + teNE) * hd.p1C) >> 5);
    prediction[2] = W - (((sumWN + teNW) * hd.p2C) >> 5);
    prediction[3] = N - ((teNW * hd.p3Ca + teN * hd.p3Cb + teNE * hd.p3Cc + (NN - N) * hd.p3Cd + (NW - W) * hd.p3Ce) >> 5);
    // WeightedAverage: weights renormalised to 4 bits + sum, division by lookup
    uint32_t weight_sum = w[0] + w[1] + w[2] + w[3];
    const uint32_t log_weight = 31 - (uint32_t)__builtin_clz(weight_sum);
    weight_sum = 0;
    for (int i = 0; i < 4; i++) {
      w[i] >>= log_weight - 4;
      weight_sum += w[i];
    }
    int64_t sum = (weight_sum >> 1) - 1;
    for (int i = 0; i < 4; i++) sum += prediction[i] * w[i];
    pred = (sum * divlookup[weight_sum - 1]) >> 24;
    if (((teN ^ teW) | (teN ^ teNW)) > 0) return (pred + kRound) >> kExtra;
    const int64_t mx = std::max(W, std::max(NE, N)), mn = std::min(W, std::min(NE, N));
    pred = std::max(mn, std::min(mx, pred));
    return (pred + kRound) >> kExtra;
  }
  inline void Update(int64_t val, size_t x, size_t y) {
    const size_t cur = (y & 1) ? 0 : xsize + 2, prev = (y & 1) ? xsize + 2 : 0;
    val *= 8;
    Col& c = st[cur + x];
    Col& n = st[prev + x + 1];
    c.err = (int32_t)(pred - val);
    for (int i = 0; i < 4; i++) {
      const uint32_t err = (uint32_t)((std::abs(prediction[i] - val) + kRound) >> kExtra);
      c.pe[i] = err;
      n.pe[i] += err;
    }
  }
};

inline int32_t ClampedGradient(int32_t n, int32_t w, int32_t l) {
  const int32_t m = std::min(n, w), M = std::max(n, w);
  const int32_t grad = (int32_t)((uint32_t)n + (uint32_t)w - (uint32_t)l);
  return l > M ? m : (l < m ? M : grad);
}

// one channel (DecodeModularChannelMAANS, encoding.cc:147-510).  The reference specialises this loop by what the tree
// asks for (encoding.cc:190-480: trees that only look at the self-correcting predictor's error -- what libjxl writes
// for the DC of a VarDCT frame --, trees without that predictor, single-leaf trees); here: the part of the tree that
// cannot be reached by THIS channel of THIS stream is cut off first (properties 0 and 1 are constants), then
//   * the self-correcting predictor runs only if the remaining subtree uses it (property 15 or predictor 6),
//   * reference properties are gathered only if the subtree uses one,
//   * a subtree whose inner nodes all test property 15 becomes a 1024-entry table from the clamped property to the leaf,
//   * pixels at least two away from the channel's edges take their neighbours without bounds tests.
// Same arithmetic, same order of reads from the bit stream: bit-identical to the general loop it replaces.
struct ChannelPlan {
  uint32_t root = 0;
  bool use_wp = false, use_refs = false, wp_only = false;
  bool wp_pure = false;  // wp_only and every leaf: self-correcting predictor, multiplier 1, offset 0
  uint32_t max_prop = 0;  // the largest property an inner node of the subtree tests
  uint32_t num_props = kNumNonrefProperties;
  std::vector<uint16_t> wp_lut;  // wp_only: leaf node of clamp(property 15, -512, 511) + 512
};

static void PlanChannel(const std::vector<MaNode>& nodes, uint32_t chan, uint32_t stream_id, ChannelPlan* p) {
  uint32_t root = 0;
  while (nodes[root].property == 0 || nodes[root].property == 1) {
    const int32_t v = nodes[root].property == 0 ? (int32_t)chan : (int32_t)stream_id;
    root = v > nodes[root].splitval ? nodes[root].lchild : nodes[root].rchild;
  }
  p->root = root;
  bool only15 = true, plain_leaves = true;
  uint32_t max_prop = 0;
  std::vector<uint32_t> stack{root};
  while (!stack.empty()) {
    const MaNode& n = nodes[stack.back()];
    stack.pop_back();
    if (n.property < 0) {
      p->use_wp |= n.predictor == 6;
      plain_leaves &= n.predictor == 6 && n.multiplier == 1 && n.offset == 0;
    } else {
      only15 &= n.property == (int32_t)kWpProperty;
      p->use_wp |= n.property == (int32_t)kWpProperty;
      max_prop = std::max<uint32_t>(max_prop, (uint32_t)n.property);
      stack.push_back(n.lchild);
      stack.push_back(n.rchild);
    }
  }
  p->use_refs = max_prop >= kNumNonrefProperties;
  p->max_prop = max_prop;
  // (the reference array is sized by the WHOLE tree, like the general loop: the property indices must agree)
  uint32_t np = kNumNonrefProperties;
  for (const MaNode& n : nodes)
    if (n.property >= 0) np = std::max<uint32_t>(np, (uint32_t)n.property + 1);
  p->num_props = kNumNonrefProperties + (np - kNumNonrefProperties + 3) / 4 * 4;
  p->wp_only = only15 && nodes[root].property >= 0 && nodes.size() < 65536;
  if (p->wp_only) {
    p->wp_lut.resize(1024);
    for (int v = -512; v < 512; v++) {
      uint32_t pos = root;
      while (nodes[pos].property >= 0) pos = v > nodes[pos].splitval ? nodes[pos].lchild : nodes[pos].rchild;
      p->wp_lut[v + 512] = (uint16_t)pos;
    }
  }
  p->wp_pure = p->wp_only && plain_leaves;
}

// ---- the self-correcting predictor's own track -- what libjxl writes for the DC of a VarDCT frame and what the
// reference decodes on a loop of its own too (encoding.cc:190-480, "wp only"): every inner node of the channel's subtree
// tests property 15, every leaf predicts with the self-correcting predictor, multiplier 1, offset 0, plain ANS.  The
// arithmetic is WpState's (context_predict.h:65-196), value for value; what differs is the bookkeeping around it:
//   * WpState::Update adds a pixel's four sub-predictor errors into the PREVIOUS row's column x + 1, and Predict sums
//     the columns x - 1, x, x + 1 of that row: a store, a reload and a three-way sum between one pixel's value and the
//     next pixel's weights.  Here the previous row keeps its own errors E; T[x] = E[x-1] + E[x] + E[x+1] is summed for
//     the whole row ahead of the serial loop (edge columns count twice, as cN stands in for cNE / cNW there), and the
//     running part is what Update would have added by then: the errors of the two pixels to the left (the last column
//     sees the left neighbour's twice -- through cN and through cNE = cN),
//   * the ANS state and the bit reader live in locals (nothing else in the loop can alias them),
//   * property 15 goes through a table straight to the clustered context,
//   * clamps and the ANS renormalisation are selects, not branches (they follow the image's noise).
// (a second copy for x86-64-v3 CPUs -- AVX2, BMI2, LZCNT: every server core since 2015 --, picked at load time: the
// loop is bound by its instruction count, and shifts that take their count from any register, a leading-zero count in
// one instruction and the four error terms side by side in one vector register make it 10 % shorter on a Zen 5 core,
// profiles/r04_wp_variants_box*.txt)
JXLHIP_X86_64_V3_CLONE
int DecodeWpPureChannel(BitReader* br_io, SymbolReader* reader, const EntropyCode& code, const MaNode* nd, uint32_t root,
                        const uint16_t* node_lut, const WpHeader& hd, ModularChannel& ch) {
  const size_t w = ch.w, h = ch.h;
  const uint8_t* cmap = code.context_map.data();
  uint8_t ctx_lut[1024];
  for (int v = 0; v < 1024; v++) ctx_lut[v] = cmap[nd[node_lut[v]].leaf_id];
  std::vector<uint32_t> Erows(2 * 4 * w, 0), T(4 * (w + 2));
  // the previous row's true errors and its samples, one copy of the edge column on either side: what Predict / the
  // property gatherer substitute there (cNW = cN at x = 0, cNE = cN at x = w - 1; topleft = left = top at x = 0,
  // topright = top at x = w - 1: context_predict.h:384-470)
  std::vector<int32_t> err_rows(2 * (w + 2), 0), up_pad(w + 2, 0);
  uint32_t divlookup[64];
  for (uint32_t i = 0; i < 64; i++) divlookup[i] = (1u << 24) / (i + 1);
  BitReader br = *br_io;
  uint32_t state = reader->State();
  const AliasEntry* const alias = code.alias.data();
  const HybridUint* const configs = code.configs.data();
  const uint32_t log_alpha = code.log_alpha, log_entry = kAnsLogTab - log_alpha, entry_mask = (1u << log_entry) - 1;
  // the weight of a sub-predictor from its recent errors (ErrorWeight, context_predict.h:111-117: a leading-zero count,
  // two shifts by it, a table and a multiply) sits between one sample and the next one's prediction: sums below
  // kWeightTable -- all but the sharpest edges of a DC image -- read it from a table made once per channel
  constexpr uint32_t kWeightTable = 512;
  uint32_t wtab[4][kWeightTable];
  for (int i = 0; i < 4; i++)
    for (uint32_t v = 0; v < kWeightTable; v++) wtab[i][v] = WpState::ErrorWeightOf(v, hd.w[i], divlookup);
  const int64_t p1C = hd.p1C, p2C = hd.p2C, p3Ca = hd.p3Ca, p3Cb = hd.p3Cb, p3Cc = hd.p3Cc, p3Cd = hd.p3Cd, p3Ce = hd.p3Ce;
  constexpr int64_t kRound = WpState::kRound;
  constexpr int kExtra = WpState::kExtra;

  for (size_t y = 0; y < h; y++) {
    int32_t* const row = ch.Row((uint32_t)y);
    uint32_t* const Ec = Erows.data() + (y & 1) * 4 * w;
    const uint32_t* const Ep = Erows.data() + ((y & 1) ^ 1) * 4 * w;
    int32_t* const errc = err_rows.data() + (y & 1) * (w + 2) + 1;
    const int32_t* const errp = err_rows.data() + ((y & 1) ^ 1) * (w + 2) + 1;
    const int32_t* const up = up_pad.data() + 1;
    const int32_t* const up2 = y > 1 ? ch.Row((uint32_t)y - 2) : up;  // (toptop = top on the second row)
    if (y) {
      memcpy(up_pad.data() + 1, ch.Row((uint32_t)y - 1), w * sizeof(int32_t));
      up_pad[0] = up_pad[1];
      up_pad[w + 1] = up_pad[w];
    }
    if (w == 1) {
      for (int i = 0; i < 4; i++) T[i] = 3u * Ep[i];
    } else {
      for (int i = 0; i < 4; i++) T[i] = 2u * Ep[i] + Ep[4 + i];
      for (size_t k = 4; k < 4 * (w - 1); k++) T[k] = Ep[k - 4] + Ep[k] + Ep[k + 4];
      for (int i = 0; i < 4; i++) T[4 * (w - 1) + i] = 2u * Ep[4 * (w - 1) + i] + Ep[4 * (w - 2) + i];
    }
    uint32_t e1_0 = 0, e1_1 = 0, e1_2 = 0, e1_3 = 0;  // the left neighbour's errors; the one before it is added into T
    int64_t teW = 0;
    int64_t W = y ? up[0] : 0;  // (left of the first column: the sample above it; nothing on the first row)

    // (every lambda below is inlined into this loop: a call would pin the state they share -- the ANS state, the bit
    // reader, the running errors -- to memory)
    auto weight = [&](uint32_t S, int i) __attribute__((always_inline)) -> uint32_t {
      if (__builtin_expect(S < kWeightTable, 1)) return wtab[i][S];
      return WpState::ErrorWeightOf(S, hd.w[i], divlookup);
    };
    auto pixel = [&](size_t x, int64_t N, int64_t NE, int64_t NW, int64_t NN, int64_t teN, int64_t teNW, int64_t teNE,
                     auto last /* std::true_type: the row's last column (of several) */) __attribute__((always_inline)) {
      const uint32_t* t = &T[4 * x];
      constexpr uint32_t twice = decltype(last)::value ? 2u : 1u;
      uint32_t w0 = weight(t[0] + twice * e1_0, 0), w1 = weight(t[1] + twice * e1_1, 1);
      uint32_t w2 = weight(t[2] + twice * e1_2, 2), w3 = weight(t[3] + twice * e1_3, 3);
      // the property: the largest (by magnitude, first wins) of the neighbours' true errors, teW first -> the context;
      // the token read can start while the prediction is still being put together
      int64_t te3 = teN;
      te3 = std::abs(teNW) > std::abs(te3) ? teNW : te3;
      te3 = std::abs(teNE) > std::abs(te3) ? teNE : te3;
      const int32_t prop = (int32_t)(std::abs(te3) > std::abs(teW) ? te3 : teW);
      uint32_t ctx;
      if ((uint32_t)(prop + 512) < 1024u) {
        ctx = ctx_lut[prop + 512];
      } else {  // beyond the table the tree may still split
        uint32_t pos = root;
        while (nd[pos].property >= 0) pos = prop > nd[pos].splitval ? nd[pos].lchild : nd[pos].rchild;
        ctx = cmap[nd[pos].leaf_id];
      }
      br.Refill();
      const uint32_t res = state & (kAnsTab - 1);
      const AliasEntry e = alias[((size_t)ctx << log_alpha) + (res >> log_entry)];
      const uint32_t pos = res & entry_mask;
      const bool right = pos >= e.cutoff;
      uint32_t token = right ? e.right_value : (res >> log_entry);
      const uint32_t offset = (right ? e.offsets1 : 0u) + pos;
      const uint32_t freq = right ? e.freq1 : e.freq0;
      const uint32_t ns = freq * (state >> kAnsLogTab) + offset;
      const bool renorm = ns < (1u << 16);
      const uint32_t refilled = (ns << 16) | (uint32_t)br.Peek(16);
      state = renorm ? refilled : ns;
      br.Consume(renorm ? 16u : 0u);
      const HybridUint& hc = configs[ctx];
      if (token >= hc.split_token) token = FinishHybridUint(hc, token, &br);

      const int64_t N8 = N * 8, W8 = W * 8, NE8 = NE * 8, NW8 = NW * 8, NN8 = NN * 8;
      const int64_t sumWN = teN + teW;
      const int64_t pr0 = W8 + NE8 - N8;
      const int64_t pr1 = N8 - (((sumWN + teNE) * p1C) >> 5);
      const int64_t pr2 = W8 - (((sumWN + teNW) * p2C) >> 5);
      const int64_t pr3 = N8 - ((teNW * p3Ca + teN * p3Cb + teNE * p3Cc + (NN8 - N8) * p3Cd + (NW8 - W8) * p3Ce) >> 5);
      uint32_t weight_sum = w0 + w1 + w2 + w3;
      const uint32_t sh = (31 - (uint32_t)__builtin_clz(weight_sum)) - 4;
      w0 >>= sh, w1 >>= sh, w2 >>= sh, w3 >>= sh;
      weight_sum = w0 + w1 + w2 + w3;
      const int64_t sum = (int64_t)((weight_sum >> 1) - 1) + pr0 * w0 + pr1 * w1 + pr2 * w2 + pr3 * w3;
      int64_t pred = (sum * divlookup[weight_sum - 1]) >> 24;
      const bool keep = ((teN ^ teW) | (teN ^ teNW)) > 0;  // (no clamp: the bounds move out of reach)
      const int64_t mx = keep ? INT64_MAX : std::max(W8, std::max(NE8, N8)), mn = keep ? INT64_MIN : std::min(W8, std::min(NE8, N8));
      pred = std::max(mn, std::min(mx, pred));
      const int64_t guess = (pred + kRound) >> kExtra;
      const int32_t val = (int32_t)(UnpackSigned64(token) + guess);
      row[x] = val;
      W = val;
      const int64_t v8 = (int64_t)val * 8;
      const int32_t te = (int32_t)(pred - v8);
      errc[x] = te;
      teW = te;
      e1_0 = (uint32_t)((std::abs(pr0 - v8) + kRound) >> kExtra);
      e1_1 = (uint32_t)((std::abs(pr1 - v8) + kRound) >> kExtra);
      e1_2 = (uint32_t)((std::abs(pr2 - v8) + kRound) >> kExtra);
      e1_3 = (uint32_t)((std::abs(pr3 - v8) + kRound) >> kExtra);
      Ec[4 * x] = e1_0, Ec[4 * x + 1] = e1_1, Ec[4 * x + 2] = e1_2, Ec[4 * x + 3] = e1_3;
      uint32_t* t2 = &T[4 * x + 8];  // (two columns on: off the critical path; T has two columns to spare)
      t2[0] += e1_0, t2[1] += e1_1, t2[2] += e1_2, t2[3] += e1_3;
    };
    const size_t xl = w - 1;
    if (y == 0) {  // every neighbour is the sample to the left; no errors above
      for (size_t x = 0; x < xl; x++) pixel(x, W, W, W, W, 0, 0, 0, std::false_type());
      if (w > 1) pixel(xl, W, W, W, W, 0, 0, 0, std::true_type());
      else pixel(xl, W, W, W, W, 0, 0, 0, std::false_type());
    } else {
      for (size_t x = 0; x < xl; x++)
        pixel(x, up[x], up[x + 1], up[(ptrdiff_t)x - 1], up2[x], errp[x], errp[(ptrdiff_t)x - 1], errp[x + 1], std::false_type());
      if (w > 1) pixel(xl, up[xl], up[xl + 1], up[(ptrdiff_t)xl - 1], up2[xl], errp[xl], errp[(ptrdiff_t)xl - 1], errp[xl + 1], std::true_type());
      else pixel(xl, up[xl], up[xl + 1], up[(ptrdiff_t)xl - 1], up2[xl], errp[xl], errp[(ptrdiff_t)xl - 1], errp[xl + 1], std::false_type());
    }
    errc[-1] = errc[0];
    errc[w] = errc[w - 1];
    if (!br.Healthy()) {
      *br_io = br;
      reader->SetState(state);
      return kBad;
    }
  }
  *br_io = br;
  reader->SetState(state);
  return kOk;
}

// ---- channels whose subtree asks for neither the self-correcting predictor nor an earlier channel (the strategy /
// quant-field / sharpness streams of a DC group, most extra-channel streams): the general loop's arithmetic
// (context_predict.h:384-545) with the ANS state and the bit reader in locals, the row above padded by the samples the
// edge rules substitute, and -- when no inner node tests a property above 7 -- only the neighbours those need.
JXLHIP_X86_64_V3_CLONE
int DecodeSimpleChannel(BitReader* br_io, SymbolReader* reader, const EntropyCode& code, const MaNode* nd, uint32_t root,
                        ModularChannel& ch, uint32_t chan, uint32_t stream_id, bool all_props) {
  const size_t w = ch.w, h = ch.h;
  const uint8_t* cmap = code.context_map.data();
  std::vector<int32_t> up_pad(w + 3, 0);
  BitReader br = *br_io;
  uint32_t state = reader->State();
  const AliasEntry* const alias = code.alias.data();
  const HybridUint* const configs = code.configs.data();
  const uint32_t log_alpha = code.log_alpha, log_entry = kAnsLogTab - log_alpha, entry_mask = (1u << log_entry) - 1;
  const bool single_leaf = nd[root].property < 0;
  int32_t P[kNumNonrefProperties] = {};
  P[0] = (int32_t)chan;
  P[1] = (int32_t)stream_id;
  for (size_t y = 0; y < h; y++) {
    int32_t* const row = ch.Row((uint32_t)y);
    const int32_t* const up = up_pad.data() + 1;
    const int32_t* const up2 = y > 1 ? ch.Row((uint32_t)y - 2) : up;
    if (y) {
      memcpy(up_pad.data() + 1, ch.Row((uint32_t)y - 1), w * sizeof(int32_t));
      up_pad[0] = up_pad[1];
      up_pad[w + 1] = up_pad[w + 2] = up_pad[w];
    }
    P[2] = (int32_t)y;
    int64_t left = y ? up[0] : 0, leftleft = left, grad = 0;
    auto pixel = [&](size_t x, auto first_row, auto every_property) __attribute__((always_inline)) {
      constexpr bool kRow0 = decltype(first_row)::value, kAllProps = decltype(every_property)::value;
      const int64_t top = kRow0 ? left : up[x], topleft = kRow0 ? left : up[(ptrdiff_t)x - 1], topright = kRow0 ? left : up[x + 1];
      int64_t toptop = 0, toprightright = 0;
      uint32_t pos = root;
      if (!single_leaf) {
        P[3] = (int32_t)x;
        P[4] = (int32_t)(top > 0 ? top : -top);
        P[5] = (int32_t)(left > 0 ? left : -left);
        P[6] = (int32_t)top;
        P[7] = (int32_t)left;
        if (kAllProps) {
          toptop = kRow0 ? left : up2[x];
          toprightright = kRow0 ? left : up[x + 2];
          P[8] = (int32_t)(left - grad);
          grad = left + top - topleft;
          P[9] = (int32_t)grad;
          P[10] = (int32_t)(left - topleft);
          P[11] = (int32_t)(topleft - top);
          P[12] = (int32_t)(top - topright);
          P[13] = (int32_t)(top - toptop);
          P[14] = (int32_t)(left - leftleft);
        }
        while (nd[pos].property >= 0) pos = P[nd[pos].property] > nd[pos].splitval ? nd[pos].lchild : nd[pos].rchild;
      }
      const MaNode& leaf = nd[pos];
      const uint32_t ctx = cmap[leaf.leaf_id];
      br.Refill();
      const uint32_t res = state & (kAnsTab - 1);
      const AliasEntry e = alias[((size_t)ctx << log_alpha) + (res >> log_entry)];
      const uint32_t apos = res & entry_mask;
      const bool right = apos >= e.cutoff;
      uint32_t token = right ? e.right_value : (res >> log_entry);
      const uint32_t offset = (right ? e.offsets1 : 0u) + apos;
      const uint32_t freq = right ? e.freq1 : e.freq0;
      const uint32_t ns = freq * (state >> kAnsLogTab) + offset;
      const bool renorm = ns < (1u << 16);
      const uint32_t refilled = (ns << 16) | (uint32_t)br.Peek(16);
      state = renorm ? refilled : ns;
      br.Consume(renorm ? 16u : 0u);
      const HybridUint& hc = configs[ctx];
      if (token >= hc.split_token) token = FinishHybridUint(hc, token, &br);
      int64_t guess;
      switch (leaf.predictor) {  // PredictOne, context_predict.h:471-510 (6, the self-correcting one, never gets here)
        case 1: guess = left; break;
        case 2: guess = top; break;
        case 3: guess = (left + top) / 2; break;
        case 4: {
          const int64_t p = left + top - topleft;
          guess = std::abs(p - left) < std::abs(p - top) ? left : top;
          break;
        }
        case 5: guess = ClampedGradient((int32_t)left, (int32_t)top, (int32_t)topleft); break;
        case 7: guess = topright; break;
        case 8: guess = topleft; break;
        case 9: guess = leftleft; break;
        case 10: guess = (left + topleft) / 2; break;
        case 11: guess = (topleft + top) / 2; break;
        case 12: guess = (top + topright) / 2; break;
        case 13:
          if (!kAllProps) {
            toptop = kRow0 ? left : up2[x];
            toprightright = kRow0 ? left : up[x + 2];
          }
          guess = (6 * top - 2 * toptop + 7 * left + leftleft + toprightright + 3 * topright + 8) / 16;
          break;
        default: guess = 0; break;
      }
      const int32_t val = (int32_t)(UnpackSigned64(token) * (int64_t)(int32_t)leaf.multiplier + leaf.offset + guess);
      row[x] = val;
      leftleft = x ? left : val;  // (the sample two to the left from the third column on; the left one before)
      left = val;
    };
    if (y == 0) {
      if (all_props) for (size_t x = 0; x < w; x++) pixel(x, std::true_type(), std::true_type());
      else for (size_t x = 0; x < w; x++) pixel(x, std::true_type(), std::false_type());
    } else {
      if (all_props) for (size_t x = 0; x < w; x++) pixel(x, std::false_type(), std::true_type());
      else for (size_t x = 0; x < w; x++) pixel(x, std::false_type(), std::false_type());
    }
    if (!br.Healthy()) {
      *br_io = br;
      reader->SetState(state);
      return kBad;
    }
  }
  *br_io = br;
  reader->SetState(state);
  return kOk;
}

int DecodeModularChannel(BitReader* br, SymbolReader* reader, const jxlhip_modular_tree& tree, const WpHeader& wph,
                         std::vector<ModularChannel>& image, uint32_t chan, uint32_t stream_id) {
  ModularChannel& ch = image[chan];
  if (ch.w == 0 || ch.h == 0) return kOk;
  const std::vector<MaNode>& nodes = tree.nodes;
  const uint8_t* cmap = tree.code.context_map.data();
  ChannelPlan plan;
  PlanChannel(nodes, chan, stream_id, &plan);
  const uint32_t num_props = plan.num_props;
  const uint32_t num_ref = plan.use_refs ? num_props - kNumNonrefProperties : 0;
  std::vector<int32_t> props(num_props, 0);
  std::vector<int32_t> refs((size_t)num_ref * ch.w);
  // earlier channels of the same size feed 4 properties each (PrecomputeReferences, context_predict.h:407-441)
  std::vector<uint32_t> ref_channels;
  for (int32_t j = (int32_t)chan - 1; j >= 0 && ref_channels.size() * 4 < num_ref; j--) {
    if (image[j].w == ch.w && image[j].h == ch.h && image[j].hshift == ch.hshift && image[j].vshift == ch.vshift)
      ref_channels.push_back((uint32_t)j);
  }
  std::unique_ptr<WpState> wp(plan.use_wp ? new WpState(wph, ch.w) : nullptr);
  const size_t w = ch.w;
  const MaNode* const nd = nodes.data();
  const uint32_t root = plan.root;
  const bool single_leaf = nd[root].property < 0;
  const uint16_t* lut = plan.wp_only ? plan.wp_lut.data() : nullptr;
  int32_t* const P = props.data();
  const bool plain_ans = !tree.code.use_prefix && !tree.code.lz77.enabled;  // (the token reader's fast track, as for AC groups)
  if (plan.wp_pure && plain_ans && !jxlhip_env::Get().wp_general.load(std::memory_order_relaxed)) {
    return DecodeWpPureChannel(br, reader, tree.code, nd, root, plan.wp_lut.data(), wph, ch);
  }
  if (!plan.use_wp && !plan.use_refs && plain_ans && !jxlhip_env::Get().wp_general.load(std::memory_order_relaxed)) {
    const int rc = DecodeSimpleChannel(br, reader, tree.code, nd, root, ch, chan, stream_id, plan.max_prop > 7);
    return rc;
  }

  // the rest of a pixel once its neighbours are known
  auto finish = [&](int32_t* row, size_t x, uint32_t y, int64_t left, int64_t top, int64_t topleft, int64_t topright,
                    int64_t leftleft, int64_t toptop, int64_t toprightright) {
    int64_t wp_pred = 0;
    if (wp) wp_pred = wp->Predict(x, y, top, left, topright, topleft, toptop, &P[kWpProperty]);
    uint32_t pos;
    if (lut) {
      const int32_t v = P[kWpProperty];
      pos = lut[(v < -512 ? -512 : (v > 511 ? 511 : v)) + 512];
      // outside the table's range the tree may still split: finish the walk from the table's node upwards is not
      // possible, so walk from the root for those (rare) values
      if (v < -512 || v > 511) {
        pos = root;
        while (nd[pos].property >= 0) pos = v > nd[pos].splitval ? nd[pos].lchild : nd[pos].rchild;
      }
    } else if (single_leaf) {
      pos = root;
    } else {
      P[3] = (int32_t)x;
      P[4] = (int32_t)(top > 0 ? top : -top);
      P[5] = (int32_t)(left > 0 ? left : -left);
      P[6] = (int32_t)top;
      P[7] = (int32_t)left;
      P[8] = (int32_t)(left - P[9]);  // against the previous pixel's gradient property
      P[9] = (int32_t)(left + top - topleft);
      P[10] = (int32_t)(left - topleft);
      P[11] = (int32_t)(topleft - top);
      P[12] = (int32_t)(top - topright);
      P[13] = (int32_t)(top - toptop);
      P[14] = (int32_t)(left - leftleft);
      if (num_ref) memcpy(&P[kNumNonrefProperties], &refs[x * num_ref], num_ref * sizeof(int32_t));
      pos = root;
      while (nd[pos].property >= 0) pos = P[nd[pos].property] > nd[pos].splitval ? nd[pos].lchild : nd[pos].rchild;
    }
    const MaNode& leaf = nd[pos];
    int64_t guess;
    switch (leaf.predictor) {  // PredictOne, context_predict.h:471-510
      case 1: guess = left; break;
      case 2: guess = top; break;
      case 3: guess = (left + top) / 2; break;
      case 4: {
        const int64_t p = left + top - topleft;
        guess = std::abs(p - left) < std::abs(p - top) ? left : top;
        break;
      }
      case 5: guess = ClampedGradient((int32_t)left, (int32_t)top, (int32_t)topleft); break;
      case 6: guess = wp_pred; break;
      case 7: guess = topright; break;
      case 8: guess = topleft; break;
      case 9: guess = leftleft; break;
      case 10: guess = (left + topleft) / 2; break;
      case 11: guess = (topleft + top) / 2; break;
      case 12: guess = (top + topright) / 2; break;
      case 13: guess = (6 * top - 2 * toptop + 7 * left + leftleft + toprightright + 3 * topright + 8) / 16; break;
      default: guess = 0; break;
    }
    const uint64_t v = plain_ans ? reader->ReadHybridUintAns(cmap[leaf.leaf_id], br) : reader->ReadHybridUint(cmap[leaf.leaf_id], br);
    row[x] = (int32_t)(UnpackSigned64(v) * (int64_t)(int32_t)leaf.multiplier + leaf.offset + guess);
    if (wp) wp->Update(row[x], x, y);
  };
  // property 9 of the PREVIOUS pixel feeds property 8: it has to be maintained even where the table / single leaf
  // path does not compute the properties -- those paths never read it, the general path recomputes it per pixel.
  for (uint32_t y = 0; y < ch.h; y++) {
    int32_t* row = ch.Row(y);
    const int32_t* up = y ? ch.Row(y - 1) : nullptr;
    const int32_t* up2 = y > 1 ? ch.Row(y - 2) : nullptr;
    for (size_t k = 0; k < ref_channels.size(); k++) {
      const ModularChannel& rc = image[ref_channels[k]];
      const int32_t* rp = rc.Row(y);
      const int32_t* rpp = rc.Row(y ? y - 1 : 0);
      for (size_t x = 0; x < w; x++) {
        const int64_t v = rp[x];
        const int64_t vleft = x ? rp[x - 1] : 0, vtop = y ? rpp[x] : vleft, vtopleft = (x && y) ? rpp[x - 1] : vleft;
        const int64_t predicted = ClampedGradient((int32_t)vleft, (int32_t)vtop, (int32_t)vtopleft);
        int32_t* o = &refs[x * num_ref + k * 4];
        o[0] = (int32_t)std::abs(v);
        o[1] = (int32_t)v;
        o[2] = (int32_t)std::abs(v - predicted);
        o[3] = (int32_t)(v - predicted);
      }
    }
    P[0] = (int32_t)chan;
    P[1] = (int32_t)stream_id;
    P[2] = (int32_t)y;
    P[9] = 0;
    auto edge = [&](size_t x) {
      const int64_t left = x ? row[x - 1] : (y ? up[x] : 0);
      const int64_t top = y ? up[x] : left;
      const int64_t topleft = (x && y) ? up[x - 1] : left;
      const int64_t topright = (x + 1 < w && y) ? up[x + 1] : top;
      const int64_t leftleft = x > 1 ? row[x - 2] : left;
      const int64_t toptop = y > 1 ? up2[x] : top;
      const int64_t toprightright = (x + 2 < w && y) ? up[x + 2] : topright;
      finish(row, x, y, left, top, topleft, topright, leftleft, toptop, toprightright);
    };
    if (y < 2 || w < 5) {
      for (size_t x = 0; x < w; x++) edge(x);
    } else {
      edge(0);
      edge(1);
      for (size_t x = 2; x + 2 < w; x++)
        finish(row, x, y, row[x - 1], up[x], up[x - 1], up[x + 1], row[x - 2], up2[x], up[x + 2]);
      edge(w - 2);
      edge(w - 1);
    }
    if (!br->Healthy()) return kBad;
  }
  return kOk;
}

// InvPalette, one channel, no delta entries, predictor Zero (palette.cc:29-75, the nb == 1 branch), last transform first
// ---- squeeze (modular/transform/squeeze.cc): a channel is split into averages of sample pairs and residuals,
// horizontally or vertically, again and again; the residual channels carry shifts one higher per split, so that the
// groups deliver them level by level ----------------------------------------------------------------------------

// DefaultSqueezeParameters (squeeze.cc:406-455): for three or more equally sized channels the 2nd and 3rd are halved
// both ways first (residuals at the end), then all channels are halved in place, the longer side first, down to 8 x 8
void DefaultSqueezeSteps(const std::vector<ModularChannel>& image, uint32_t nb_meta, std::vector<SqueezeStep>* steps) {
  steps->clear();
  const uint32_t nb = (uint32_t)image.size() - nb_meta;
  uint32_t w = image[nb_meta].w, h = image[nb_meta].h;
  SqueezeStep q;
  if (nb > 2 && image[nb_meta + 1].w == w && image[nb_meta + 1].h == h) {
    q.in_place = false;
    q.begin_c = nb_meta + 1;
    q.num_c = 2;
    q.horizontal = true;
    steps->push_back(q);
    q.horizontal = false;
    steps->push_back(q);
  }
  q.begin_c = nb_meta;
  q.num_c = nb;
  q.in_place = true;
  auto halve = [&](bool horizontal) {
    q.horizontal = horizontal;
    steps->push_back(q);
    uint32_t& side = horizontal ? w : h;
    side = (side + 1) / 2;
  };
  if (w <= h && h > 8) halve(false);
  while (w > 8 || h > 8) {
    if (w > 8) halve(true);
    if (h > 8) halve(false);
  }
}

// MetaSqueeze (squeeze.cc:457-514): the channel list after the forward transform -- shapes and shifts only
int MetaSqueeze(std::vector<ModularChannel>& image, uint32_t* nb_meta, std::vector<SqueezeStep>* steps) {
  if (steps->empty()) {
    if (image.size() <= *nb_meta) return kBad;
    DefaultSqueezeSteps(image, *nb_meta, steps);
  }
  for (const SqueezeStep& q : *steps) {
    const uint64_t first = q.begin_c, last = (uint64_t)q.begin_c + q.num_c - 1;
    if (q.num_c == 0 || last >= image.size()) return kBad;
    if (first < *nb_meta) {
      if (last >= *nb_meta || !q.in_place) return kBad;
      *nb_meta += q.num_c;
    }
    const size_t at = q.in_place ? (size_t)last + 1 : image.size();
    for (uint32_t c = (uint32_t)first; c <= last; c++) {
      ModularChannel& ch = image[c];
      if (ch.hshift > 30 || ch.vshift > 30 || ch.w == 0 || ch.h == 0) return kBad;
      ModularChannel res;
      if (q.horizontal) {
        res.Shape(ch.w - (ch.w + 1) / 2, ch.h);
        ch.Shape((ch.w + 1) / 2, ch.h);
        if (ch.hshift >= 0) ch.hshift++;
      } else {
        res.Shape(ch.w, ch.h - (ch.h + 1) / 2);
        ch.Shape(ch.w, (ch.h + 1) / 2);
        if (ch.vshift >= 0) ch.vshift++;
      }
      res.hshift = ch.hshift;
      res.vshift = ch.vshift;
      image.insert(image.begin() + at + (c - (uint32_t)first), std::move(res));
    }
  }
  return kOk;
}

// What the pair (average, residual) is expected to differ by, from the sample before the pair, the pair's average
// and the next average: zero unless the three are monotonic (SmoothTendency, squeeze.h:60-77)
inline int64_t SqueezeTendency(int64_t before, int64_t avg, int64_t next) {
  int64_t d = 0;
  if (before >= avg && avg >= next) {
    d = (4 * before - 3 * next - avg + 6) / 12;
    if (d - (d & 1) > 2 * (before - avg)) d = 2 * (before - avg) + 1;
    if (d + (d & 1) > 2 * (avg - next)) d = 2 * (avg - next);
  } else if (before <= avg && avg <= next) {
    d = (4 * before - 3 * next - avg - 6) / 12;
    if (d + (d & 1) < 2 * (before - avg)) d = 2 * (before - avg) - 1;
    if (d - (d & 1) < 2 * (avg - next)) d = 2 * (avg - next);
  }
  return d;
}

// InvHSqueeze / InvVSqueeze (squeeze.cc:126-233, 235-317): `avg` and its residual channel become the channel of
// twice the size along one axis
// (`spread(n, task)` runs task(0..n-1), possibly on several threads: rows are independent in the horizontal case,
// columns in the vertical one -- 8-row / 64-column tasks like the reference's, squeeze.cc:171-228,262-303)
typedef std::function<void(uint32_t, const std::function<void(uint32_t)>&)> TaskSpreader;
int UnsqueezePair(ModularChannel& avg, const ModularChannel& res, bool horizontal, const TaskSpreader& spread) {
  if (avg.w < res.w || avg.h < res.h) return kBad;
  if (horizontal ? (avg.h != res.h || avg.w != (avg.w + res.w + 1) / 2) : (avg.w != res.w || avg.h != (avg.h + res.h + 1) / 2))
    return kBad;
  if (avg.px.size() != (size_t)avg.w * avg.h || res.px.size() != (size_t)res.w * res.h) return kBad;
  ModularChannel out;
  out.hshift = avg.hshift - (horizontal ? 1 : 0);
  out.vshift = avg.vshift - (horizontal ? 0 : 1);
  if (horizontal) {
    if (res.w == 0) {  // nothing was split off
      avg.hshift--;
      return kOk;
    }
    out.Resize(avg.w + res.w, avg.h);
    spread((avg.h + 7) / 8, [&](uint32_t task) {
    for (uint32_t y = task * 8; y < std::min(avg.h, task * 8 + 8); y++) {
      const int32_t* a = avg.Row(y);
      const int32_t* r = res.Row(y);
      int32_t* o = out.Row(y);
      for (uint32_t x = 0; x < res.w; x++) {
        const int64_t v = a[x], next = x + 1 < avg.w ? a[x + 1] : v, left = x ? o[2 * x - 1] : v;
        const int64_t diff = r[x] + SqueezeTendency(left, v, next);
        const int64_t first = v + diff / 2;
        o[2 * x] = (int32_t)first;
        o[2 * x + 1] = (int32_t)(first - diff);
      }
      if (out.w & 1) o[out.w - 1] = a[avg.w - 1];
    }
    });
  } else {
    if (res.h == 0) {
      avg.vshift--;
      return kOk;
    }
    out.Resize(avg.w, avg.h + res.h);
    spread((avg.w + 63) / 64, [&](uint32_t task) {
    const uint32_t x0 = task * 64, x1 = std::min(avg.w, task * 64 + 64);
    for (uint32_t y = 0; y < res.h; y++) {
      const int32_t* a = avg.Row(y);
      const int32_t* an = avg.Row(y + 1 < avg.h ? y + 1 : y);
      const int32_t* r = res.Row(y);
      int32_t* o = out.Row(2 * y);
      int32_t* on = out.Row(2 * y + 1);
      const int32_t* above = y ? out.Row(2 * y - 1) : a;
      for (uint32_t x = x0; x < x1; x++) {
        const int64_t v = a[x];
        const int64_t diff = r[x] + SqueezeTendency(above[x], v, an[x]);
        const int64_t first = v + diff / 2;
        o[x] = (int32_t)first;
        on[x] = (int32_t)(first - diff);
      }
    }
    });
    if (out.h & 1) memcpy(out.Row(out.h - 1), avg.Row(avg.h - 1), (size_t)avg.w * sizeof(int32_t));
  }
  avg = std::move(out);
  return kOk;
}

// InvSqueeze (squeeze.cc:319-360): the steps undone last to first; residual channels leave the list
inline void SerialTasks(uint32_t n, const std::function<void(uint32_t)>& task) {
  for (uint32_t i = 0; i < n; i++) task(i);
}
int UndoSqueeze(std::vector<ModularChannel>& image, uint32_t* nb_meta, const std::vector<SqueezeStep>& steps,
                const TaskSpreader& spread = SerialTasks) {
  for (size_t i = steps.size(); i-- > 0;) {
    const SqueezeStep& q = steps[i];
    const uint64_t first = q.begin_c, last = (uint64_t)q.begin_c + q.num_c - 1;
    if (q.num_c == 0 || last >= image.size()) return kBad;
    const uint64_t at = q.in_place ? last + 1 : image.size() - q.num_c;
    if (at + q.num_c > image.size() || at <= last) return kBad;
    if (first < *nb_meta) {
      if (*nb_meta <= q.num_c) return kBad;
      *nb_meta -= q.num_c;
    }
    for (uint32_t c = (uint32_t)first; c <= last; c++) {
      const int rc = UnsqueezePair(image[c], image[(size_t)at + c - (uint32_t)first], q.horizontal, spread);
      if (rc) return rc;
    }
    image.erase(image.begin() + (size_t)at, image.begin() + (size_t)at + q.num_c);
  }
  return kOk;
}

// A palette index outside the table (palette.h:53-122): negative = one of 143 signed deltas, size .. size + 63 = a
// 4 x 4 x 4 colour cube, beyond = a 5 x 5 x 5 one, both scaled to the image's bit depth; channels past the third are 0.
// libjxl's encoder leaves the colours that sit on those cubes out of the tables it writes, lossless palettes included
inline int32_t PaletteValue(const int32_t* table, int32_t index, uint32_t c, int32_t size, uint32_t bit_depth) {
  static const int16_t kDelta[72][3] = {
      {0, 0, 0},       {4, 4, 4},       {11, 0, 0},      {0, 0, -13},     {0, -12, 0},     {-10, -10, -10},
      {-18, -18, -18}, {-27, -27, -27}, {-18, -18, 0},   {0, 0, -32},     {-32, 0, 0},     {-37, -37, -37},
      {0, -32, -32},   {24, 24, 45},    {50, 50, 50},    {-45, -24, -24}, {-24, -45, -45}, {0, -24, -24},
      {-34, -34, 0},   {-24, 0, -24},   {-45, -45, -24}, {64, 64, 64},    {-32, 0, -32},   {0, -32, 0},
      {-32, 0, 32},    {-24, -45, -24}, {45, 24, 45},    {24, -24, -45},  {-45, -24, 24},  {80, 80, 80},
      {64, 0, 0},      {0, 0, -64},     {0, -64, -64},   {-24, -24, 45},  {96, 96, 96},    {64, 64, 0},
      {45, -24, -24},  {34, -34, 0},    {112, 112, 112}, {24, -45, -45},  {45, 45, -24},   {0, -32, 32},
      {24, -24, 45},   {0, 96, 96},     {45, -24, 24},   {24, -45, -24},  {-24, -45, 24},  {0, -64, 0},
      {96, 0, 0},      {128, 128, 128}, {64, 0, 64},     {144, 144, 144}, {96, 96, 0},     {-36, -36, 36},
      {45, -24, -45},  {45, -45, -24},  {0, 0, -96},     {0, 128, 128},   {0, 96, 0},      {45, 24, -45},
      {-128, 0, 0},    {24, -45, 24},   {-45, 24, -45},  {64, 0, -64},    {64, -64, -64},  {96, 0, 96},
      {45, -45, 24},   {24, 45, -45},   {64, 64, -64},   {128, 128, 0},   {0, 0, -128},    {-24, 45, -45}};
  if (index >= 0 && index < size) return table[(size_t)c * size + index];
  if (c >= 3) return 0;
  if (index < 0) {
    int32_t i = -(index + 1);
    i %= 143;
    const uint32_t e = (uint32_t)(i + 1) >> 1;
    int32_t v = kDelta[e][c];
    if (!(i & 1)) v = -v;
    if (bit_depth > 8) v *= (int32_t)1 << (bit_depth - 8);
    return v;
  }
  const uint64_t top = ((uint64_t)1 << bit_depth) - 1;
  uint32_t i = (uint32_t)(index - size);
  if (i < 64) return (int32_t)((((i >> (2 * c)) % 4) * top) >> 2) + (1 << (bit_depth > 3 ? bit_depth - 3 : 0));
  i -= 64;
  if (c == 1) i /= 5;
  if (c == 2) i /= 25;
  return (int32_t)(((i % 5) * top) >> 2);
}

// InvRCT (rct.cc:29-148) on channels begin_c .. begin_c + 2, in place: type = 7 * permutation + custom; custom 6 is
// YCoCg, otherwise bit 0 adds the first channel to the third and the bits above add the first (1) or the average of
// the first and the third (2) to the second; the permutation says where the three results go.  int32 arithmetic that
// wraps, like the reference's Add / PixelAdd, and its arithmetic >> 1.
inline void InvRctPixel(uint32_t custom, int32_t* a, int32_t* b, int32_t* c) {
  const uint32_t first = (uint32_t)*a, second = (uint32_t)*b, third = (uint32_t)*c;
  if (custom == 6) {
    const uint32_t tmp = first - (uint32_t)((int32_t)third >> 1);  // Y - (Cg >> 1)
    const uint32_t g = third + tmp;
    const uint32_t bl = tmp - (uint32_t)((int32_t)second >> 1);
    *a = (int32_t)(bl + second);
    *b = (int32_t)g;
    *c = (int32_t)bl;
    return;
  }
  uint32_t s2 = second, s3 = third;
  if (custom & 1) s3 += first;
  if ((custom >> 1) == 1) s2 += first;
  else if ((custom >> 1) == 2) s2 += (uint32_t)((int32_t)(first + s3) >> 1);
  *b = (int32_t)s2;
  *c = (int32_t)s3;
}
int UndoRct(std::vector<ModularChannel>& image, uint32_t begin_c, uint32_t type) {
  if ((uint64_t)begin_c + 2 >= image.size() || type >= 42) return kBad;
  ModularChannel* ch = &image[begin_c];
  const size_t n = (size_t)ch[0].w * ch[0].h;
  for (int i = 0; i < 3; i++)
    if (ch[i].w != ch[0].w || ch[i].h != ch[0].h || ch[i].px.size() != n) return kBad;
  if (type == 0) return kOk;
  const uint32_t perm = type / 7, custom = type % 7;
  const uint32_t to[3] = {perm % 3, (perm + 1 + perm / 3) % 3, (perm + 2 - perm / 3) % 3};
  int32_t* out[3] = {ch[to[0]].px.data(), ch[to[1]].px.data(), ch[to[2]].px.data()};
  const int32_t *in0 = ch[0].px.data(), *in1 = ch[1].px.data(), *in2 = ch[2].px.data();
  for (size_t i = 0; i < n; i++) {
    int32_t a = in0[i], b = in1[i], c = in2[i];  // (all three are read before any is written: out is a permutation of in)
    InvRctPixel(custom, &a, &b, &c);
    out[0][i] = a;
    out[1][i] = b;
    out[2][i] = c;
  }
  return kOk;
}

// InvPalette without deltas (palette.cc:29-100), last transform first: the index channel becomes num_c channels
// again; one-channel palettes clamp the index into the table, the others use the implicit entries
int UndoPalettes(std::vector<ModularChannel>& image, std::vector<ModularPalette>& palettes, uint32_t* nb_meta,
                 uint32_t image_bits) {
  const uint32_t bit_depth = std::min<uint32_t>(image_bits, 24);
  while (!palettes.empty()) {
    if (palettes.back().rct) {
      const int rc = UndoRct(image, palettes.back().begin_c, palettes.back().rct_type);
      if (rc) return rc;
      palettes.pop_back();
      continue;
    }
    const uint32_t c0 = palettes.back().begin_c + 1;
    if (*nb_meta < 1 || c0 >= image.size()) return kBad;
    const uint32_t nb = image[0].h;
    const int32_t size = (int32_t)image[0].w;
    if (nb < 1 || image[0].px.size() != (size_t)nb * image[0].w) return kBad;
    if (nb == 1) {
      const int32_t* lut = image[0].px.data();
      const int32_t last = size - 1;
      // (an empty table: the clamped index is -1, the first -- zero -- delta entry)
      for (int32_t& v : image[c0].px) v = size ? lut[v < 0 ? 0 : (v > last ? last : v)] : 0;
    } else {
      if (bit_depth == 0) return JXLHIP_ERR_UNSUPPORTED;  // (the caller did not say what the image's bit depth is)
      if (image[c0].px.size() != (size_t)image[c0].w * image[c0].h) return kBad;
      ModularChannel shape;
      shape.Resize(image[c0].w, image[c0].h);
      shape.hshift = image[c0].hshift;
      shape.vshift = image[c0].vshift;
      image.insert(image.begin() + c0 + 1, nb - 1, shape);
      const int32_t* table = image[0].px.data();
      const size_t n = image[c0].px.size();
      for (uint32_t c = nb; c-- > 0;) {  // channel 0 holds the indices: overwritten last
        int32_t* out = image[c0 + c].px.data();
        const int32_t* idx = image[c0].px.data();
        for (size_t i = 0; i < n; i++) out[i] = PaletteValue(table, idx[i], c, size, bit_depth);
      }
    }
    if (c0 >= *nb_meta) {
      (*nb_meta)--;
    } else {  // a palette of meta channels: nb of them are back, the table goes
      if ((int64_t)*nb_meta < 2 - (int64_t)nb) return kBad;
      *nb_meta = (uint32_t)((int64_t)*nb_meta - (2 - (int64_t)nb));
    }
    image.erase(image.begin());
    palettes.pop_back();
  }
  return kOk;
}

struct PendingTransforms {  // of the frame's global image, until every group is in (FinalizeDecoding)
  std::vector<ModularPalette> palettes;
  ModularSqueeze squeeze;  // behind the palettes: undone first
  uint32_t nb_meta = 0;
};

// ModularDecode + ModularGenericDecompress (encoding.cc:553-726): group header, MetaApply of its (single-channel
// palette) transforms, the tree, every channel up to the first non-meta one larger than max_chan_size, then the
// transforms undone.  The frame's GLOBAL image (max_chan_size = the group size, `pending` given) may leave channels
// to the groups: its transforms then stay in *pending, with the meta channels in front of the image, until every
// group is in (FinalizeDecoding, dec_modular.cc:739-760).
int ModularDecodeImage(BitReader* br, std::vector<ModularChannel>& image, uint32_t stream_id,
                       const jxlhip_modular_tree* global, uint32_t max_chan_size, uint32_t image_bits,
                       PendingTransforms* pending = nullptr, const std::function<int(uint32_t)>* after_channel = nullptr,
                       bool allow_lz77 = false, const char** why = nullptr, ModularStreamOptions* opt = nullptr) {
  // allow_lz77: an entropy code with LZ77 is read with the 2-D special distances (jxlhip_modular_frame_decode; the
  // other callers keep refusing it).  why: where JXLHIP_ERR_UNSUPPORTED came from, as a static string.
  // opt: the stream belongs to a regular Modular frame (ModularStreamOptions).
  // after_channel(c): channel c's samples are final -- called between the channels of a stream WITHOUT transforms only
  // (with a palette or a squeeze nothing is final before the end); a non-zero return stops the decode with that status
  if (image.empty()) return kOk;  // not even a group header (encoding.cc:558)
  bool use_global_tree;
  WpHeader wp;
  std::vector<ModularPalette> palettes;
  ModularSqueeze squeeze;
  allow_lz77 = allow_lz77 || (opt && opt->lz77);
  int rc = ReadModularGroupHeader(br, &use_global_tree, &wp, &palettes, pending ? &squeeze : nullptr, opt && opt->rct);
  if (rc == JXLHIP_ERR_UNSUPPORTED && why)
    *why = opt && opt->rct ? "a delta palette, or a squeeze inside a group's stream or in front of another transform"
                           : "a transform of the Modular frame (RCT, squeeze, delta palette)";
  if (rc) return rc;
  if (opt) opt->transforms = !palettes.empty() || squeeze.present;
  // the hand-over rule of a regular Modular frame: nothing but RCTs over the three colour channels, which lead the image
  bool leave = opt && opt->leave_rcts && !squeeze.present && opt->channels >= 3 && image.size() == opt->channels && !palettes.empty() &&
               palettes.size() <= kMaxDeviceRcts;
  for (const ModularPalette& t : palettes) leave = leave && t.rct && t.begin_c == 0;
  // MetaPalette with begin_c == end_c (palette.cc:171-200): the palette becomes channel 0 (nb_colors x 1, shifts -1),
  // the channel itself now holds indices
  // (several channels, begin_c .. begin_c + num_c - 1, of one shape share a table of num_c rows and leave ONE index
  // channel, palette.cc:177-200; CheckEqualChannels transform.cc:146-165)
  uint32_t nb_meta = 0;
  for (const ModularPalette& t : palettes) {
    const uint64_t first = t.begin_c, last = first + t.num_c - 1;
    if (t.num_c == 0 || last >= image.size() || (first < nb_meta && last >= nb_meta)) return kBad;
    for (uint64_t c = first + 1; c <= last; c++)
      if (image[c].w != image[first].w || image[c].h != image[first].h || image[c].hshift != image[first].hshift ||
          image[c].vshift != image[first].vshift)
        return kBad;
    if (t.rct) continue;  // (an RCT changes no shape: its MetaApply is that check, transform.cc:112-114)
    if (first >= nb_meta) nb_meta++;
    else nb_meta = nb_meta + 2 - t.num_c;  // (last < nb_meta: at least one stays)
    image.erase(image.begin() + (size_t)first + 1, image.begin() + (size_t)last + 1);
    ModularChannel pal;
    pal.Resize(t.nb_colors, t.num_c);
    pal.hshift = pal.vshift = -1;
    image.insert(image.begin(), std::move(pal));
  }
  if (squeeze.present && (rc = MetaSqueeze(image, &nb_meta, &squeeze.steps))) return rc;
  auto stops = [&](uint32_t i) { return i >= nb_meta && (image[i].w > max_chan_size || image[i].h > max_chan_size); };
  bool complete = true;
  for (uint32_t i = 0; i < image.size(); i++) complete &= !stops(i);
  if (!palettes.empty() && !complete && !pending) return JXLHIP_ERR_UNSUPPORTED;
  if (squeeze.present) {  // the shapes are new: samples for what this section decodes (the groups allocate theirs)
    for (uint32_t i = 0; i < image.size() && !stops(i); i++) image[i].Resize(image[i].w, image[i].h);
  }
  auto undo = [&]() -> int {
    if (leave) {  // the device undoes them per pixel (k_modular_emit), last-listed first
      opt->left = true;
      opt->program = (uint16_t)(palettes[0].rct_type | (palettes.size() > 1 ? palettes[1].rct_type << 8 : 0u));
      return kOk;
    }
    // (a squeezed global image stays squeezed even when this section held all of it: the groups look for THEIR
    // channels in the squeezed list and find none, dec_modular.cc:344-350; FinalizeDecoding undoes it)
    if (pending && (!complete || squeeze.present)) {  // the groups fill the rest first
      pending->palettes = palettes;
      pending->squeeze = squeeze;
      pending->nb_meta = nb_meta;
      return kOk;
    }
    if (squeeze.present && (rc = UndoSqueeze(image, &nb_meta, squeeze.steps))) return rc;
    return UndoPalettes(image, palettes, &nb_meta, image_bits);
  };
  uint64_t pixels = 0;
  size_t num_chans = 0;
  uint32_t distance_multiplier = 0;  // the widest channel this stream holds (encoding.cc:590-604)
  for (uint32_t i = 0; i < image.size(); i++) {
    if (stops(i)) break;
    const ModularChannel& c = image[i];
    if (c.w && c.h) {
      num_chans++;
      distance_multiplier = std::max(distance_multiplier, c.w);
    }
    pixels += (uint64_t)c.w * c.h;
  }
  if (num_chans == 0) return undo();
  jxlhip_modular_tree local;
  const jxlhip_modular_tree* tree = global;
  if (!use_global_tree) {
    if ((rc = DecodeMaTree(br, (size_t)std::min<uint64_t>(1u << 20, 1024 + pixels), &local))) {
      if (rc == JXLHIP_ERR_UNSUPPORTED && why) *why = "the MA tree of the Modular frame";
      return rc;
    }
    tree = &local;
  } else if (!global || global->nodes.empty()) {
    return kBad;
  }
  if (tree->code.lz77.enabled && !allow_lz77) return JXLHIP_ERR_UNSUPPORTED;  // 2-D special distances
  SymbolReader reader(&tree->code, br);
  if (!reader.Ok()) return JXLHIP_ERR_OUT_OF_MEMORY;
  reader.SetDistanceMultiplier(distance_multiplier);
  for (uint32_t c = 0; c < image.size(); c++) {
    if (stops(c)) break;
    if ((rc = DecodeModularChannel(br, &reader, *tree, wp, image, c, stream_id))) return rc;
    if (after_channel && palettes.empty() && !squeeze.present && (rc = (*after_channel)(c))) return rc;
  }
  if (reader.Corrupt() || !reader.FinalStateOk() || !br->Healthy()) return kBad;
  return undo();
}

int ModularDecodePlain(BitReader* br, std::vector<ModularChannel>& image, uint32_t stream_id,
                       const jxlhip_modular_tree* global, uint32_t image_bits,
                       const std::function<int(uint32_t)>* after_channel = nullptr) {
  return ModularDecodeImage(br, image, stream_id, global, 0xFFFFFFu, image_bits, nullptr, after_channel);
}

// ModularFrameDecoder's full_image for the extra channels of a VarDCT frame (dec_modular.cc:207-316)
struct ModularFull {
  std::vector<ModularChannel> ch;  // one per extra channel, behind the meta channels of the pending transforms
  PendingTransforms pending;
  uint32_t group_dim = 256, xsg = 1, num_groups = 1, num_dc_groups = 1;
  uint32_t image_bits = 0;  // ImageMetadata::bit_depth.bits_per_sample (implicit palette entries scale with it)
  // channels larger than a group are filled by the AC groups: their int32 planes are only allocated for the callers
  // that collect them here (jxlhip_modular_ac_group_decode); jxlhip_modular_ac_group_decode_f32 writes the float
  // samples straight into the caller's planes
  std::once_flag alloc_once;
  // the first non-meta channel larger than a group: it and everything behind it (after a squeeze: residual channels
  // of every size) comes with the groups (DecodeGroup, dec_modular.cc:344-350)
  uint32_t FirstGroupChannel() const {
    uint32_t c = pending.nb_meta;
    while (c < ch.size() && ch[c].w <= group_dim && ch[c].h <= group_dim) c++;
    return c;
  }
  void AllocateLarge() {
    std::call_once(alloc_once, [this] {
      for (uint32_t c = FirstGroupChannel(); c < ch.size(); c++)
        if (ch[c].px.empty()) ch[c].px.assign((size_t)ch[c].w * ch[c].h, 0);
    });
  }
};

}  // namespace

// DecodeGlobalInfo (dec_modular.cc:207-316) of a VarDCT frame: the optional global tree and the global Modular
// image -- empty without extra channels; with them (alpha, depth, ...: frame->num_extra_channels <= 4, each at the
// frame's resolution) its group header, transforms and every channel that fits one group.  The larger channels
// arrive with the AC groups (jxlhip_modular_ac_group_decode).
static int ModularGlobalDecodeImpl(const uint8_t* data, size_t size, size_t* bit_pos, const jxlhip_frame_header* fh,
                                   jxlhip_modular_tree** out);
// (the extra channels' planes are header-sized host allocations: a failure comes back as a status)
int jxlhip_modular_global_decode(const uint8_t* data, size_t size, size_t* bit_pos, const jxlhip_frame_header* fh,
                                 jxlhip_modular_tree** out) {
  try {
    return ModularGlobalDecodeImpl(data, size, bit_pos, fh, out);
  } catch (const std::bad_alloc&) {
    if (out) *out = nullptr;
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}
static int ModularGlobalDecodeImpl(const uint8_t* data, size_t size, size_t* bit_pos, const jxlhip_frame_header* fh,
                                   jxlhip_modular_tree** out) {
  if (!data || !bit_pos || !fh || !out) return JXLHIP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  // (an upsampled frame without extra channels has an empty global image like any other)
  if (fh->is_modular || fh->num_extra_channels > 4 || (fh->upsampling != 1 && fh->num_extra_channels != 0))
    return JXLHIP_ERR_UNSUPPORTED;
  for (uint32_t i = 0; i < fh->num_extra_channels; i++)
    if (fh->ec_upsampling[i] != 1) return JXLHIP_ERR_UNSUPPORTED;
  BitReader br(data, size, *bit_pos);
  std::unique_ptr<jxlhip_modular_tree> t;
  const uint32_t nb_extra = fh->num_extra_channels;
  const bool has_tree = br.Read(1) != 0;
  if (has_tree || nb_extra) {
    t.reset(new (std::nothrow) jxlhip_modular_tree);
    if (!t) return JXLHIP_ERR_OUT_OF_MEMORY;
  }
  if (has_tree) {
    const uint64_t limit = std::min<uint64_t>(1u << 22, 1024 + (uint64_t)fh->xsize * fh->ysize * (3 + nb_extra) / 16);
    const int rc = DecodeMaTree(&br, (size_t)limit, t.get());
    if (rc) return rc;
  }
  if (nb_extra) {
    t->full = std::make_shared<ModularFull>();
    ModularFull& f = *t->full;
    f.group_dim = fh->group_dim;
    f.xsg = fh->xsize_groups;
    f.num_groups = (uint32_t)fh->num_groups;
    f.num_dc_groups = (uint32_t)fh->num_dc_groups;
    f.image_bits = fh->image_bits;
    f.ch.resize(nb_extra);
    if ((uint64_t)fh->xsize * fh->ysize * nb_extra > ((uint64_t)1 << 32)) return JXLHIP_ERR_OUT_OF_MEMORY;
    const bool large = fh->xsize > fh->group_dim || fh->ysize > fh->group_dim;
    for (ModularChannel& c : f.ch) {
      if (large) c.Shape(fh->xsize, fh->ysize);  // left to the groups
      else c.Resize(fh->xsize, fh->ysize);
    }
    const int rc = ModularDecodeImage(&br, f.ch, 0, t.get(), fh->group_dim, fh->image_bits, &f.pending);
    if (rc) return rc;
  }
  if (!br.Healthy()) return kBad;
  *bit_pos = br.BitsConsumed();
  *out = t.release();
  return kOk;
}

// Passes::GetDownsamplingBracket (frame_header.h:268-284)
static void DownsamplingBracket(const jxlhip_frame_header* fh, uint32_t pass, int* min_shift, int* max_shift) {
  int mx = 2, mn = 3;
  for (uint32_t i = 0;; i++) {
    for (uint32_t j = 0; j < fh->num_downsample; j++) {
      if (i == fh->last_pass[j]) {
        if (fh->downsample[j] == 8) mn = 3;
        if (fh->downsample[j] == 4) mn = 2;
        if (fh->downsample[j] == 2) mn = 1;
        if (fh->downsample[j] == 1) mn = 0;
      }
    }
    if (i == fh->num_passes - 1) mn = 0;
    if (i == pass) break;
    mx = mn - 1;
  }
  *min_shift = mn;
  *max_shift = mx;
}

// ModularFrameDecoder::DecodeGroup for ModularStreamId::ModularAC(group, pass) (dec_modular.cc:330-425): what
// follows the VarDCT coefficients in pass `pass` of AC group `group` -- the group's rectangle of every
// extra channel larger than a group.  Thread-safe for different groups.
static int ModularAcGroupDecodeImpl(jxlhip_modular_tree* global, const jxlhip_frame_header* fh, uint32_t group,
                                    uint32_t pass, const uint8_t* data, size_t size, size_t* bit_pos);
int jxlhip_modular_ac_group_decode(jxlhip_modular_tree* global, const jxlhip_frame_header* fh, uint32_t group,
                                   uint32_t pass, const uint8_t* data, size_t size, size_t* bit_pos) {
  try {
    return ModularAcGroupDecodeImpl(global, fh, group, pass, data, size, bit_pos);
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}
// the group's rectangles of the large channels, decoded: gi[i] belongs to channel which[i] of the full image
// (DecodeGroup's rectangle x0, y0, dim x dim in frame pixels, its shift bracket and stream)
static int ModularGroupRects(const jxlhip_modular_tree* global, uint32_t x0, uint32_t y0, uint32_t dim, int min_shift,
                             int max_shift, uint32_t stream_id, const uint8_t* data, size_t size, size_t* bit_pos,
                             std::vector<ModularChannel>* gi, std::vector<uint32_t>* which,
                             ModularStreamOptions* opt = nullptr) {
  ModularFull& f = *global->full;
  for (uint32_t c = f.FirstGroupChannel(); c < f.ch.size(); c++) {
    const ModularChannel& fc = f.ch[c];
    const int shift = std::min(fc.hshift, fc.vshift);
    if (shift > max_shift || shift < min_shift) continue;
    const uint32_t rx = x0 >> fc.hshift, ry = y0 >> fc.vshift;
    if (rx >= fc.w || ry >= fc.h) continue;
    const uint32_t rw = std::min(dim >> fc.hshift, fc.w - rx), rh = std::min(dim >> fc.vshift, fc.h - ry);
    if (rw == 0 || rh == 0) continue;
    ModularChannel gc;
    gc.Resize(rw, rh);
    gc.hshift = fc.hshift;
    gc.vshift = fc.vshift;
    gi->push_back(std::move(gc));
    which->push_back(c);
  }
  if (gi->empty()) return kOk;
  BitReader br(data, size, *bit_pos);
  const int rc = ModularDecodeImage(&br, *gi, stream_id, global, 0xFFFFFFu, f.image_bits, nullptr, nullptr, false, nullptr, opt);
  if (rc) return rc;
  if (!br.Healthy() || gi->size() != which->size()) return kBad;
  for (size_t i = 0; i < which->size(); i++) {
    const ModularChannel& fc = f.ch[(*which)[i]];
    const ModularChannel& gc = (*gi)[i];
    const uint32_t rx = x0 >> fc.hshift, ry = y0 >> fc.vshift;
    if (gc.w > fc.w - rx || gc.h > fc.h - ry) return kBad;
  }
  *bit_pos = br.BitsConsumed();
  return kOk;
}
static void ModularGroupCopy(ModularFull& f, uint32_t x0, uint32_t y0, const std::vector<ModularChannel>& gi,
                             const std::vector<uint32_t>& which) {
  f.AllocateLarge();
  for (size_t i = 0; i < which.size(); i++) {
    ModularChannel& fc = f.ch[which[i]];
    const ModularChannel& gc = gi[i];
    const uint32_t rx = x0 >> fc.hshift, ry = y0 >> fc.vshift;
    for (uint32_t y = 0; y < gc.h; y++) memcpy(fc.Row(ry + y) + rx, gc.Row(y), gc.w * sizeof(int32_t));
  }
}
static int ModularAcGroupRects(jxlhip_modular_tree* global, const jxlhip_frame_header* fh, uint32_t group, uint32_t pass,
                               const uint8_t* data, size_t size, size_t* bit_pos, std::vector<ModularChannel>* gi,
                               std::vector<uint32_t>* which) {
  const ModularFull& f = *global->full;
  int min_shift, max_shift;
  DownsamplingBracket(fh, pass, &min_shift, &max_shift);
  return ModularGroupRects(global, (group % f.xsg) * f.group_dim, (group / f.xsg) * f.group_dim, f.group_dim, min_shift,
                           max_shift, 1 + 3 * f.num_dc_groups + 17 + f.num_groups * pass + group, data, size, bit_pos, gi,
                           which);
}

static int ModularAcGroupDecodeImpl(jxlhip_modular_tree* global, const jxlhip_frame_header* fh, uint32_t group,
                                    uint32_t pass, const uint8_t* data, size_t size, size_t* bit_pos) {
  if (!fh || !data || !bit_pos) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!global || !global->full) return fh->num_extra_channels ? JXLHIP_ERR_STATE : kOk;
  ModularFull& f = *global->full;
  if (group >= f.num_groups || pass >= fh->num_passes) return JXLHIP_ERR_INVALID_ARGUMENT;
  std::vector<ModularChannel> gi;
  std::vector<uint32_t> which;
  const int rc = ModularAcGroupRects(global, fh, group, pass, data, size, bit_pos, &gi, &which);
  if (rc || gi.empty()) return rc;
  ModularGroupCopy(f, (group % f.xsg) * f.group_dim, (group / f.xsg) * f.group_dim, gi, which);
  return kOk;
}

// The same, with the samples converted on the spot (what FinalizeDecoding + ModularImageToDecodedRect would make of
// them, see jxlhip_modular_extra_channel_f32) and written into the caller's float planes: planes[e] for extra
// channel e (NULL = not wanted), rows of stride_floats.  The frame's int32 image is never allocated, the
// conversion runs on the group's thread.  Pending global palettes are applied here (their tables are complete once
// the global section is decoded).  JXLHIP_ERR_UNSUPPORTED: a pending palette of a palette (use the collecting form).
int jxlhip_modular_ac_group_decode_f32(jxlhip_modular_tree* global, const jxlhip_frame_header* fh, uint32_t group,
                                       uint32_t pass, const uint8_t* data, size_t size, size_t* bit_pos,
                                       const uint32_t* ec_bits, uint32_t image_bits, float* const* planes,
                                       size_t stride_floats) {
  const size_t strides[4] = {stride_floats, stride_floats, stride_floats, stride_floats};
  return jxlhip_modular_ac_group_decode_f32_strided(global, fh, group, pass, data, size, bit_pos, ec_bits, image_bits,
                                                    planes, strides);
}
// (planes with rows of their own: a pinned staging plane next to the caller's)
int jxlhip_modular_ac_group_decode_f32_strided(jxlhip_modular_tree* global, const jxlhip_frame_header* fh, uint32_t group,
                                               uint32_t pass, const uint8_t* data, size_t size, size_t* bit_pos,
                                               const uint32_t* ec_bits, uint32_t image_bits, float* const* planes,
                                               const size_t* strides_floats) {
  if (!fh || !data || !bit_pos || !ec_bits || !planes || !strides_floats) return JXLHIP_ERR_INVALID_ARGUMENT;
  if (!global || !global->full) return fh->num_extra_channels ? JXLHIP_ERR_STATE : kOk;
  try {
    ModularFull& f = *global->full;
    if (group >= f.num_groups || pass >= fh->num_passes) return JXLHIP_ERR_INVALID_ARGUMENT;
    if (f.pending.squeeze.present) return JXLHIP_ERR_UNSUPPORTED;  // the samples exist only after FinalizeDecoding
    for (const ModularPalette& t : f.pending.palettes)
      if (t.num_c != 1) return JXLHIP_ERR_UNSUPPORTED;  // one index channel for several extra channels
    const uint32_t P = (uint32_t)f.pending.palettes.size();
    if (P != f.pending.nb_meta) return kBad;
    for (uint32_t k = 0; k < P; k++)
      if (f.pending.palettes[k].begin_c + 1 + (P - 1 - k) < P) return JXLHIP_ERR_UNSUPPORTED;  // its target is a palette
    std::vector<ModularChannel> gi;
    std::vector<uint32_t> which;
    const int rc = ModularAcGroupRects(global, fh, group, pass, data, size, bit_pos, &gi, &which);
    if (rc || gi.empty()) return rc;
    const uint32_t x0 = (group % f.xsg) * f.group_dim, y0 = (group / f.xsg) * f.group_dim;
    for (size_t i = 0; i < which.size(); i++) {
      const uint32_t j = which[i], e = j - P;  // position in the image / extra channel index
      if (e >= fh->num_extra_channels || !planes[e]) continue;
      ModularChannel& gc = gi[i];
      // InvPalette (one channel, no deltas), last transform first; palette k's table sits at position P - 1 - k
      for (uint32_t k = P; k-- > 0;) {
        if (f.pending.palettes[k].begin_c + 1 + (P - 1 - k) != j) continue;
        const ModularChannel& pal = f.ch[P - 1 - k];
        if (pal.h != 1 || pal.px.size() != (size_t)pal.w) return kBad;
        const int32_t last = (int32_t)pal.w - 1;
        // (an empty table -- nb_colors = 0 is legal -- : the clamped index is -1, the first, zero, delta entry; as UndoPalettes)
        const int32_t* lut = pal.w ? pal.Row(0) : nullptr;
        for (int32_t& v : gc.px) v = lut ? lut[v < 0 ? 0 : (v > last ? last : v)] : 0;
      }
      const size_t stride_floats = strides_floats[e];
      if (ec_bits[e] == 0 || ec_bits[e] >= 32 || stride_floats < f.ch[j].w) return JXLHIP_ERR_INVALID_ARGUMENT;
      const double factor = 1.0 / (double)((1u << ec_bits[e]) - 1);
      const float factor_f = (float)factor;
      const uint32_t rx = x0 >> gc.hshift, ry = y0 >> gc.vshift;
      for (uint32_t y = 0; y < gc.h; y++) {
        const int32_t* in = gc.Row(y);
        float* o = planes[e] + (size_t)(ry + y) * stride_floats + rx;
        if (image_bits < 23) {
          for (uint32_t x = 0; x < gc.w; x++) o[x] = (float)in[x] * factor_f;
        } else {
          for (uint32_t x = 0; x < gc.w; x++) o[x] = (float)(in[x] * factor);
        }
      }
    }
    return kOk;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

// FinalizeDecoding + ModularImageToDecodedRect for one extra channel (dec_modular.cc:686-737,739-760): the global
// image's pending transforms are undone (once), then integer samples -> float, v * (1 / (2^bits - 1)) in float, or
// in double when the IMAGE's bit depth is 23 or more (SingleFromSingle / SingleFromSingleAccurate, :92-124).
// Not thread-safe.
int jxlhip_modular_extra_channel_f32(jxlhip_modular_tree* global, uint32_t ec, uint32_t ec_bits, uint32_t image_bits,
                                     float* out, size_t stride_floats) {
  if (!global || !global->full || !out || ec_bits == 0 || ec_bits >= 32) return JXLHIP_ERR_INVALID_ARGUMENT;
  ModularFull& f = *global->full;
  try {
    if (f.pending.squeeze.present) {
      const int rc = UndoSqueeze(f.ch, &f.pending.nb_meta, f.pending.squeeze.steps);
      if (rc) return rc;
      f.pending.squeeze = ModularSqueeze();
    }
    const int rc = UndoPalettes(f.ch, f.pending.palettes, &f.pending.nb_meta, f.image_bits ? f.image_bits : image_bits);
    if (rc) return rc;
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
  if (f.pending.nb_meta != 0 || ec >= f.ch.size()) return JXLHIP_ERR_INVALID_ARGUMENT;
  const ModularChannel& ch = f.ch[ec];
  if (ch.px.size() != (size_t)ch.w * ch.h) return JXLHIP_ERR_STATE;  // (its groups went through the _f32 form)
  if (stride_floats < ch.w) return JXLHIP_ERR_INVALID_ARGUMENT;
  const double factor = 1.0 / (double)((1u << ec_bits) - 1);
  const float factor_f = (float)factor;
  for (uint32_t y = 0; y < ch.h; y++) {
    const int32_t* in = ch.Row(y);
    float* o = out + (size_t)y * stride_floats;
    if (image_bits < 23) {
      for (uint32_t x = 0; x < ch.w; x++) o[x] = (float)in[x] * factor_f;
    } else {
      for (uint32_t x = 0; x < ch.w; x++) o[x] = (float)(in[x] * factor);
    }
  }
  return kOk;
}

// FinalizeDecoding's undo_transforms (dec_modular.cc:739-760) with the caller's threads: the squeeze pyramid level by
// level, every level spread over the runner; then the palettes (serial).  Afterwards jxlhip_modular_extra_channel_f32
// / _rows_f32 only convert.
namespace {
struct SpreadJob {
  const std::function<void(uint32_t)>* task;
};
int SpreadInit(void*, size_t) { return 0; }
void SpreadFunc(void* opaque, uint32_t i, size_t) { (*static_cast<SpreadJob*>(opaque)->task)(i); }
}  // namespace
int jxlhip_modular_finalize(jxlhip_modular_tree* global, jxlhip_parallel_runner runner, void* runner_opaque) {
  if (!global || !global->full) return kOk;
  ModularFull& f = *global->full;
  try {
    bool runner_failed = false;
    const TaskSpreader spread = [&](uint32_t n, const std::function<void(uint32_t)>& task) {
      if (!runner || n < 2) return SerialTasks(n, task);
      SpreadJob job{&task};
      if (runner(runner_opaque, &job, SpreadInit, SpreadFunc, 0, n) != 0) runner_failed = true;
    };
    if (f.pending.squeeze.present) {
      const int rc = UndoSqueeze(f.ch, &f.pending.nb_meta, f.pending.squeeze.steps, spread);
      if (rc) return rc;
      if (runner_failed) return JXLHIP_ERR_STATE;
      f.pending.squeeze = ModularSqueeze();
    }
    if (f.image_bits == 0 && !f.pending.palettes.empty())
      for (const ModularPalette& t : f.pending.palettes)
        if (t.num_c != 1) return JXLHIP_ERR_UNSUPPORTED;
    return UndoPalettes(f.ch, f.pending.palettes, &f.pending.nb_meta, f.image_bits);
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}

// rows [y0, y1) of extra channel `ec` after jxlhip_modular_finalize (JXLHIP_ERR_STATE before it); thread-safe
int jxlhip_modular_extra_channel_rows_f32(const jxlhip_modular_tree* global, uint32_t ec, uint32_t ec_bits,
                                          uint32_t image_bits, uint32_t y0, uint32_t y1, float* out, size_t stride_floats) {
  if (!global || !global->full || !out || ec_bits == 0 || ec_bits >= 32) return JXLHIP_ERR_INVALID_ARGUMENT;
  const ModularFull& f = *global->full;
  if (f.pending.squeeze.present || !f.pending.palettes.empty() || f.pending.nb_meta != 0) return JXLHIP_ERR_STATE;
  if (ec >= f.ch.size()) return JXLHIP_ERR_INVALID_ARGUMENT;
  const ModularChannel& ch = f.ch[ec];
  if (ch.px.size() != (size_t)ch.w * ch.h) return JXLHIP_ERR_STATE;
  if (stride_floats < ch.w || y0 > y1 || y1 > ch.h) return JXLHIP_ERR_INVALID_ARGUMENT;
  const double factor = 1.0 / (double)((1u << ec_bits) - 1);
  const float factor_f = (float)factor;
  for (uint32_t y = y0; y < y1; y++) {
    const int32_t* in = ch.Row(y);
    float* o = out + (size_t)y * stride_floats;
    if (image_bits < 23) {
      for (uint32_t x = 0; x < ch.w; x++) o[x] = (float)in[x] * factor_f;
    } else {
      for (uint32_t x = 0; x < ch.w; x++) o[x] = (float)(in[x] * factor);
    }
  }
  return kOk;
}

int jxlhip_modular_groups_are_final(const jxlhip_modular_tree* tree) {
  if (!tree || !tree->full) return 1;
  const ModularFull& f = *tree->full;
  if (f.pending.squeeze.present) return 0;
  for (const ModularPalette& t : f.pending.palettes)
    if (t.num_c != 1) return 0;
  const uint32_t P = (uint32_t)f.pending.palettes.size();
  for (uint32_t k = 0; k < P; k++)
    if (f.pending.palettes[k].begin_c + 1 + (P - 1 - k) < P) return 0;  // a palette of a palette
  return 1;
}

int jxlhip_modular_uses_dc_groups(const jxlhip_modular_tree* tree) {
  return tree && tree->full && tree->full->pending.squeeze.present ? 1 : 0;
}

void jxlhip_modular_tree_destroy(jxlhip_modular_tree* tree) { delete tree; }

// ProcessDCGroup (dec_frame.cc:318-342) of a VarDCT frame: DecodeVarDCTDC, (no modular DC image), DecodeAcMetadata
int jxlhip_dc_group_decode(const jxlhip_modular_tree* global, const uint8_t* data, size_t size, size_t* bit_pos,
                           const jxlhip_frame_header* fh, uint32_t dc_group, int32_t* const quant_dc[3],
                           uint32_t* extra_precision, uint8_t* ac_strategy, int32_t* raw_quant, uint8_t* epf_sharpness,
                           int8_t* ytox_map, int8_t* ytob_map, uint32_t* used_acs) {
  return jxlhip_dc_group_decode_staged(global, data, size, bit_pos, fh, dc_group, quant_dc, extra_precision, ac_strategy, raw_quant,
                                       epf_sharpness, ytox_map, ytob_map, used_acs, nullptr, nullptr);
}

int jxlhip_dc_group_decode_staged(const jxlhip_modular_tree* global, const uint8_t* data, size_t size, size_t* bit_pos,
                                  const jxlhip_frame_header* fh, uint32_t dc_group, int32_t* const quant_dc[3],
                                  uint32_t* extra_precision, uint8_t* ac_strategy, int32_t* raw_quant, uint8_t* epf_sharpness,
                                  int8_t* ytox_map, int8_t* ytob_map, uint32_t* used_acs, void (*block_info_ready)(void*),
                                  void* ready_opaque) {
  if (!data || !bit_pos || !fh || !quant_dc || !quant_dc[0] || !quant_dc[1] || !quant_dc[2] || !ac_strategy ||
      !raw_quant || !epf_sharpness || !ytox_map || !ytob_map)
    return JXLHIP_ERR_INVALID_ARGUMENT;
  if (fh->is_modular || fh->num_extra_channels > 4 || (fh->flags & JXLHIP_FLAG_USE_DC_FRAME) || fh->chroma_mode[0] || fh->chroma_mode[1] ||
      fh->chroma_mode[2])
    return JXLHIP_ERR_UNSUPPORTED;
  for (uint32_t i = 0; i < fh->num_extra_channels; i++)
    if (fh->ec_upsampling[i] != 1) return JXLHIP_ERR_UNSUPPORTED;
  const uint32_t xsb = fh->xsize_blocks, ysb = fh->ysize_blocks, gd = fh->group_dim;  // a DC group: gd x gd blocks
  const uint32_t xdg = (xsb + gd - 1) / gd;
  if ((uint64_t)dc_group >= fh->num_dc_groups) return JXLHIP_ERR_INVALID_ARGUMENT;
  const uint32_t x0 = (dc_group % xdg) * gd, y0 = (dc_group / xdg) * gd;
  const uint32_t rw = std::min(gd, xsb - x0), rh = std::min(gd, ysb - y0);
  BitReader br(data, size, *bit_pos);
  // ---- DecodeVarDCTDC: channel 0 = Y, 1 = X, 2 = B ----
  const uint32_t precision = br.Read(2);
  if (extra_precision) *extra_precision = precision;
  std::vector<ModularChannel> image(3);
  for (ModularChannel& c : image) c.Resize(rw, rh);
  int rc = ModularDecodePlain(&br, image, 1 + dc_group, global, fh->image_bits);
  if (rc) return rc;
  for (int c = 0; c < 3; c++) {
    const ModularChannel& ch = image[c < 2 ? c ^ 1 : c];
    for (uint32_t y = 0; y < rh; y++) memcpy(quant_dc[c] + (size_t)(y0 + y) * xsb + x0, ch.Row(y), rw * sizeof(int32_t));
  }
  // ---- ModularDC (dec_frame.cc:330-337): the DC group's rectangle of every extra-channel sub-channel whose shift is 3
  // or more -- what a squeeze leaves of them at 1:8 and below; nothing is coded for unsqueezed channels ----
  if (global && global->full) {
    ModularFull& f = *global->full;
    std::vector<ModularChannel> gi;
    std::vector<uint32_t> which;
    size_t pos = br.BitsConsumed();
    rc = ModularGroupRects(global, x0 * 8, y0 * 8, gd * 8, 3, 1000, 1 + (uint32_t)fh->num_dc_groups + dc_group, data, size,
                           &pos, &gi, &which);
    if (rc) return rc;
    if (!gi.empty()) {
      ModularGroupCopy(f, x0 * 8, y0 * 8, gi, which);
      br = BitReader(data, size, pos);
    }
  }
  // ---- DecodeAcMetadata: YtoX, YtoB per 8x8 blocks; (strategy, quant) per varblock; sharpness per block ----
  const uint32_t count = br.Read(CeilLog2(rw * rh)) + 1;
  const uint32_t cx0 = x0 >> 3, cy0 = y0 >> 3, cw = (rw + 7) >> 3, chh = (rh + 7) >> 3;
  image.assign(4, ModularChannel());
  image[0].Resize(cw, chh);
  image[1].Resize(cw, chh);
  image[0].hshift = image[0].vshift = image[1].hshift = image[1].vshift = 3;  // (never reference channels of [3])
  image[2].Resize(count, 2);
  image[3].Resize(rw, rh);
  // the strategy map and the quant field of the rectangle, from channel 2 alone (count x 2: strategies, quants): what
  // the AC groups under this DC group read.  Run as soon as that channel is in -- the sharpness channel behind it
  // (rw x rh samples, a tenth of the group's decode time) only matters to the loop filter -- and announced to the
  // caller (block_info_ready): its AC groups may start while this call goes on.
  bool block_info_done = false;
  uint32_t used = 0;
  auto block_info = [&]() -> int {
    block_info_done = true;
    for (uint32_t y = 0; y < rh; y++) memset(ac_strategy + (size_t)(y0 + y) * xsb + x0, 0xFF, rw);  // "not yet covered"
    const int32_t* strategies = image[2].Row(0);
    const int32_t* quants = image[2].Row(1);
    uint32_t num = 0;
    for (uint32_t iy = 0; iy < rh; iy++) {
      for (uint32_t ix = 0; ix < rw; ix++) {
        const uint32_t x = x0 + ix, y = y0 + iy;
        if (ac_strategy[(size_t)y * xsb + x] != 0xFF) continue;
        if (num >= count) return kBad;
        const int32_t s = strategies[num];
        if (s < 0 || s >= 27) return kBad;
        used |= 1u << s;
        const uint32_t cx = kCovX[s], cy = kCovY[s];
        // a varblock stays inside its 32x32-block AC group and inside the frame
        if (x + cx > (x / 32 + 1) * 32 || x + cx > std::min(xsb, x0 + rw)) return kBad;
        if (y + cy > (y / 32 + 1) * 32 || y + cy > std::min(ysb, y0 + rh)) return kBad;
        for (uint32_t by = 0; by < cy; by++) {
          for (uint32_t bx = 0; bx < cx; bx++) {
            uint8_t& cell = ac_strategy[(size_t)(y + by) * xsb + x + bx];
            if (cell != 0xFF) return kBad;  // "Invalid AC strategy: block overlap" (ac_strategy.h:227-241)
            cell = (uint8_t)((s << 1) | ((bx | by) == 0));
          }
        }
        raw_quant[(size_t)y * xsb + x] = 1 + std::max(0, std::min(255, quants[num]));
        num++;
      }
    }
    if (used_acs) __atomic_fetch_or(used_acs, used, __ATOMIC_RELAXED);  // shared across the runner's DC-group tasks
    if (block_info_ready) block_info_ready(ready_opaque);
    return kOk;
  };
  const std::function<int(uint32_t)> after_channel = [&](uint32_t chan) -> int { return chan == 2 ? block_info() : kOk; };
  rc = ModularDecodePlain(&br, image, 1 + 2 * (uint32_t)fh->num_dc_groups + dc_group, global, fh->image_bits, &after_channel);
  if (rc) return rc;
  if (!block_info_done && (rc = block_info())) return rc;  // (a stream with transforms: nothing was final before its end)
  const uint32_t cstride = (xsb + 7) >> 3;
  for (uint32_t y = 0; y < chh; y++) {
    for (uint32_t x = 0; x < cw; x++) {
      ytox_map[(size_t)(cy0 + y) * cstride + cx0 + x] = (int8_t)std::min(127, std::max(-128, image[0].Row(y)[x]));
      ytob_map[(size_t)(cy0 + y) * cstride + cx0 + x] = (int8_t)std::min(127, std::max(-128, image[1].Row(y)[x]));
    }
  }
  for (uint32_t iy = 0; iy < rh; iy++) {
    const int32_t* sharp = image[3].Row(iy);
    uint8_t* out = epf_sharpness + (size_t)(y0 + iy) * xsb + x0;
    for (uint32_t ix = 0; ix < rw; ix++) {
      if (sharp[ix] < 0 || sharp[ix] >= 8) return kBad;
      out[ix] = (uint8_t)sharp[ix];
    }
  }
  if (!br.Healthy()) return kBad;
  *bit_pos = br.BitsConsumed();
  return kOk;
}

// ---- a Modular-coded frame of one group: the reference frame of a patch dictionary ------------------------------
// FrameDecoder::ProcessDCGlobal of a Modular frame (dec_frame.cc:268-302: DequantMatrices::DecodeDC only),
// ModularFrameDecoder::DecodeGlobalInfo with the colour channels (dec_modular.cc:209-318) and
// ModularImageToDecodedRect for XYB (dec_modular.cc:564-632 with MultiplySum, :61-73).  A frame of one group has all
// its samples in the global stream: its DC-group, AC-global and AC-group parts read nothing (dec_modular.cc:344-350).
static int ModularFrameDecodeImpl(const uint8_t* data, size_t size, size_t* bit_pos, const jxlhip_frame_header* fh,
                                  float* const planes[3], size_t stride_floats, const char** why) {
  auto refuse = [&](const char* what) {
    if (why) *why = what;
    return JXLHIP_ERR_UNSUPPORTED;
  };
  if (why) *why = "";
  if (!data || !bit_pos || !fh || !planes || !planes[0] || !planes[1] || !planes[2] || !fh->is_modular || fh->xsize == 0 ||
      fh->ysize == 0 || stride_floats < fh->xsize)
    return JXLHIP_ERR_INVALID_ARGUMENT;
  if (fh->color_transform != JXLHIP_CT_XYB) return refuse("a Modular frame that is not XYB");
  if (fh->num_groups != 1 || fh->xsize > fh->group_dim || fh->ysize > fh->group_dim)
    return refuse("a Modular frame of more than one group");
  if (fh->flags != 0) return refuse("a Modular frame with flags (noise, patches, splines, a DC frame)");
  if (fh->lf.gab || fh->lf.epf_iters) return refuse("a Modular frame with a loop filter");
  if (fh->upsampling != 1) return refuse("an upsampled Modular frame");
  if (fh->num_passes != 1) return refuse("a Modular frame of more than one pass");
  if (fh->dc_level != 0) return refuse("a Modular DC frame");
  if (!fh->save_before_color_transform) return refuse("a Modular frame saved behind the colour transform");
  if (fh->num_extra_channels != 0) return refuse("a Modular frame of an image with extra channels");
  BitReader br(data, size, *bit_pos);
  float dc_quant[3] = {1.0f / 4096.0f, 1.0f / 512.0f, 1.0f / 256.0f};  // DequantMatrices::DecodeDC
  if (!br.Read(1)) {
    for (float& q : dc_quant) {
      float v;
      if (!ReadF16(&br, &v)) return kBad;
      v *= 1.0f / 128.0f;
      if (v < 1e-8f) return kBad;
      q = v;
    }
  }
  if (!br.Healthy()) return kBad;
  jxlhip_modular_tree tree;
  if (br.Read(1)) {  // has_tree
    const uint64_t limit = std::min<uint64_t>(1u << 22, 1024 + (uint64_t)fh->xsize * fh->ysize * 3 / 16);
    const int rc = DecodeMaTree(&br, (size_t)limit, &tree);
    if (rc == JXLHIP_ERR_UNSUPPORTED) return refuse("the MA tree of the Modular frame");
    if (rc) return rc;
  }
  std::vector<ModularChannel> image(3);
  for (ModularChannel& c : image) c.Resize(fh->xsize, fh->ysize);
  const char* where = "a Modular feature outside this front-end";
  const int rc = ModularDecodeImage(&br, image, 0, &tree, fh->group_dim, fh->image_bits, nullptr, nullptr, /*allow_lz77=*/true,
                                    &where);
  if (rc == JXLHIP_ERR_UNSUPPORTED) return refuse(where);
  if (rc) return rc;
  if (!br.Healthy() || image.size() != 3) return kBad;
  for (const ModularChannel& c : image)
    if (c.w != fh->xsize || c.h != fh->ysize) return kBad;
  // coded as Y, X, B - Y
  for (uint32_t y = 0; y < fh->ysize; y++) {
    const int32_t *r0 = image[0].Row(y), *r1 = image[1].Row(y), *r2 = image[2].Row(y);
    float* ox = planes[0] + (size_t)y * stride_floats;
    float* oy = planes[1] + (size_t)y * stride_floats;
    float* ob = planes[2] + (size_t)y * stride_floats;
    for (uint32_t x = 0; x < fh->xsize; x++) {
      ox[x] = (float)r1[x] * dc_quant[0];
      oy[x] = (float)r0[x] * dc_quant[1];
      ob[x] = (float)(int32_t)((uint32_t)r2[x] + (uint32_t)r0[x]) * dc_quant[2];  // MultiplySum: the sum in int32
    }
  }
  *bit_pos = br.BitsConsumed();
  return kOk;
}

int jxlhip_modular_frame_decode(const uint8_t* data, size_t size, size_t* bit_pos, const jxlhip_frame_header* fh,
                                float* const planes[3], size_t stride_floats, const char** why) {
  try {
    return ModularFrameDecodeImpl(data, size, bit_pos, fh, planes, stride_floats, why);
  } catch (const std::bad_alloc&) {
    return JXLHIP_ERR_OUT_OF_MEMORY;
  }
}
