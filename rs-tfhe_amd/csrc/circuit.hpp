// circuit.hpp -- levelised circuits behind the C ABI (included by tfhe_hip.hip after pool.hpp; needs tfhe_hip_ctx,
// launch_blind_rotate, launch_key_switch and the pool's _dev entries).
//
// A circuit is a DAG over wires: the caller's inputs, then one wire per added node.  Node kinds and the reference
// operation each one equals word for word:
//   gate(op, a, b)                      Gates::<op> (src/gates.rs:54-150), op a tfhe_hip_gate code
//   mux(a, b, c)                        Gates::mux (src/gates.rs:157-183): and(a, b), and(not(a), c) without key switch,
//                                       their sum bootstrapped as or()
//   pbs(ca, a, cb, b, cconst, lut)      a programmable bootstrap (src/bootstrap/lut.rs:79-99) of ca*a + cb*b + cconst
//   pbs_many(..., lut, k)               k consecutive wires: the k functions a packed table holds, from ONE blind
//                                       rotation (tfhe_hip_batch_lincomb_bootstrap_many)
//   lincomb / not / constant            TLWE additions and scalings (src/tlwe.rs, src/gates.rs:202-219): no bootstrap
// compile() levelises it: inputs are level 0, a bootstrap sits one level above its deepest operand and a linear node at
// the level of its deepest operand.  Wires are renumbered into STORE SLOTS, level by level: inputs take slots
// 0 .. n_inputs-1 and each level's outputs one contiguous range, so that every launch writes its results contiguously
// and the store [slots][B][n+1] needs no scatter.  Per level, in this order:
//   at most one lincomb launch (k_circuit_lincomb): the linear operands a bootstrap cannot fold
//   at most one bootstrap-without-key-switch launch: the and / and(not) halves of the level's muxes
//   at most one key-switched gate launch (per-ciphertext gate codes): gates and the muxes' or()
//   one launch per (lut, coefficients, k) group of programmable bootstraps; a many-LUT group's slots are
//   function-major (node q, function j at base + j * nodes + q), so the kernel's [k][count] result is the store as it is
// The bootstraps read their operands straight out of the store: the blind rotation's prologue takes per-ciphertext
// row indices (BlindRotateArgs::idx_a / idx_b), built once per (circuit, context, B) and kept on the device.
// A bootstrap whose operands are linear nodes takes them into its own prologue (ca*a + cb*b + cconst, exact wrapping
// arithmetic) when the expanded combination has at most two source wires; otherwise they are materialised first.

namespace {

// out[r][col] = sum_t coef[t] * wires[src[t] * batch + j][col] (+ cst[node] on the body), r = node * batch + j:
// the linear nodes of a level, and (one term, coefficient 1) the indexed copy of wires out of the store
__global__ void k_circuit_lincomb(const uint32_t *wires, const uint32_t *__restrict__ off, const uint32_t *__restrict__ coef,
                                  const uint32_t *__restrict__ src, const uint32_t *__restrict__ cst, uint32_t batch,
                                  uint32_t width, uint32_t *out, size_t total) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t row = idx / width;
    const uint32_t col = (uint32_t)(idx - row * width);
    const uint32_t node = (uint32_t)(row / batch), j = (uint32_t)(row - (size_t)node * batch);
    uint32_t v = (cst && col == width - 1) ? cst[node] : 0u;
    for (uint32_t t = off[node]; t < off[node + 1]; ++t) v += coef[t] * wires[((size_t)src[t] * batch + j) * width + col];
    out[idx] = v;
  }
}

enum CircKind : uint8_t { CN_INPUT, CN_GATE, CN_MUX, CN_PBS, CN_LIN };
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kGateTv = 0xFFFFFFFFu;  // "lut" of a folded gate: the key's own test vector

struct CircExp {  // a linear form over stored wires: sum coef * wire + k (terms sorted by wire, no zero coefficient)
  std::vector<std::pair<uint32_t, uint32_t>> t;
  uint32_t k = 0;
};

struct CircNode {
  CircKind kind = CN_INPUT;
  uint8_t op = 0;
  uint32_t a = 0, b = 0, c = 0;
  uint32_t ca = 0, cb = 0, cc = 0, lut = 0;
  CircExp exp;  // CN_LIN only
  int level = 0;
  // many-LUT bootstraps (CN_PBS): nl = k functions, this wire is function fn of the node whose first wire is `head`;
  // nl = 0 for an ordinary bootstrap
  uint8_t nl = 0, fn = 0;
  uint32_t head = 0;
};

enum CircLaunchKind { CL_LINCOMB = 0, CL_NKS = 1, CL_GATE = 2, CL_LUT = 3 };
struct CircLaunch {
  int kind = CL_GATE;
  uint32_t out_slot = 0, nodes = 0;
  std::vector<uint32_t> sa, sb;  // bootstraps: operand slots per node
  std::vector<uint8_t> code;     // gate / nks launches: tfhe_hip_gate per node
  uint32_t lut = kGateTv, ca = 0, cb = 0, cc = 0;  // CL_LUT
  uint32_t n_luts = 0;                              // CL_LUT: many-LUT group of k functions (0: one function)
  std::vector<uint32_t> off, coef, src, cst;      // CL_LINCOMB: CSR over slots, per node
};
struct CircLevel {
  uint32_t begin = 0, end = 0;
  std::vector<CircLaunch> launches;
};

// What a run keeps on one device for one batch size (built once, then reused: a repeated run uploads only its inputs)
struct CircDevLaunch {
  const uint32_t *ia = nullptr, *ib = nullptr, *tv = nullptr;
  const uint8_t *code = nullptr;
  const uint32_t *off = nullptr, *coef = nullptr, *src = nullptr, *cst = nullptr;  // lincomb
  const uint32_t *ga_off = nullptr, *ga_coef = nullptr, *ga_src = nullptr, *gb_src = nullptr;  // pool: operand gathers
};
// A context's plans are used under that context's lock only; a pool's (its home member's, kept apart) under run_mu:
// a pool run takes the home member's lock one call at a time, so two runs through the pool -- or through two key views
// of it, which run on the same members -- would otherwise interleave their enqueues into the shared staging and store.
struct CircPlan {
  int device = 0;
  size_t B = 0;
  bool pool = false;
  uint64_t last_use = 0;
  DevArray<void> blob, blob8;
  std::vector<std::vector<CircDevLaunch>> lv;
  size_t max_count = 0;
  DevBuf store, stage_a, stage_b, gather;  // host-array runs: the store; pool runs: staging; gathers: their CSR
  std::vector<uint32_t> gather_key;
  std::vector<size_t> gather_offs;
  OwnEvent gather_done;  // recorded after each gather: the CSR is rewritten only once it has been read
  bool gather_recorded = false;
  std::mutex run_mu;                 // pool plans: one run at a time, prepare through the last level (and the gather)
  OwnEvent run_done;    // pool plans: recorded at the end of a run; the next run's stream waits for it
  bool run_recorded = false;
  ~CircPlan() {
    DeviceGuard dg(device);  // (the plan's device is current while its buffers and events go)
    for (DevBuf *b : {(DevBuf *)&blob, (DevBuf *)&blob8, &store, &stage_a, &stage_b, &gather}) b->release();
    gather_done.reset();
    run_done.reset();
  }
};
constexpr size_t kCircMaxPlans = 4;  // per circuit: the least recently used one beyond this is dropped
// the runtime's name for the default stream in event calls (they fault on the hipStreamLegacy handle)
inline hipStream_t circ_rt_stream(hipStream_t s) { return s == hipStreamLegacy ? (hipStream_t) nullptr : s; }

}  // namespace

struct tfhe_hip_circuit {
  uint32_t n_inputs = 0;
  std::vector<CircNode> nodes;             // one per wire
  std::vector<std::vector<uint32_t>> luts;  // [2][N] each
  bool compiled = false;
  std::vector<uint32_t> slot;      // per wire: its store slot (kNoSlot: a linear node, evaluated where it is read)
  std::vector<uint32_t> mat_slot;  // per wire: the slot a materialised linear node was written to (kNoSlot: none)
  std::vector<std::vector<uint32_t>> opnd;  // per wire: the slots its bootstrap launch(es) read
  uint32_t slots = 0;
  std::vector<CircLevel> levels;   // [0] = the inputs
  std::mutex mu;                   // construction, compilation, plan lookup
  // (context id, B, pool run): a run holds its plan's shared_ptr, so dropping one from here never frees it under a run
  std::map<std::tuple<uint64_t, size_t, bool>, std::shared_ptr<CircPlan>> plans;
  uint64_t plan_tick = 0;
};

namespace {

CircExp circ_expand(const tfhe_hip_circuit *c, uint32_t w) {
  if (c->nodes[w].kind == CN_LIN) return c->nodes[w].exp;
  CircExp e;
  e.t.push_back({w, 1u});
  return e;
}
bool circ_plain(const CircExp &e) { return e.k == 0 && e.t.size() == 1 && e.t[0].second == 1u; }
// x += s * y (wrapping; like terms merged, zero coefficients dropped)
void circ_axpy(CircExp &x, uint32_t s, const CircExp &y) {
  std::map<uint32_t, uint32_t> m(x.t.begin(), x.t.end());
  for (auto &t : y.t) m[t.first] += s * t.second;
  x.t.clear();
  for (auto &t : m)
    if (t.second) x.t.push_back(t);
  x.k += s * y.k;
}
int circ_level_of(const tfhe_hip_circuit *c, const CircExp &e) {
  int l = 0;
  for (auto &t : e.t) l = std::max(l, c->nodes[t.first].level);
  return l;
}
bool circ_wire_ok(const tfhe_hip_circuit *c, uint32_t w) { return w < c->nodes.size(); }

int circ_push(tfhe_hip_circuit *c, CircNode n, uint32_t *wire) {
  if (c->nodes.size() >= 0x7FFFFFFFu) return TFHE_HIP_EINVAL;
  c->nodes.push_back(std::move(n));
  if (wire) *wire = (uint32_t)c->nodes.size() - 1;
  return TFHE_HIP_OK;
}

// ---- compile -------------------------------------------------------------------------------------------------
struct CircOperand {  // a bootstrap's operand row: a stored wire, or a linear node materialised for it
  uint32_t wire = 0;
  bool mat = false;
};
struct CircDecision {
  int kind = CL_GATE;
  uint8_t code = 0;
  uint32_t lut = kGateTv, ca = 0, cb = 0, cc = 0;
  CircOperand x, y;
};

// the operand row for `w` as a bootstrap of level `L` reads it: a stored wire, a linear node that is a plain alias of
// one, or a linear node to materialise (earliest consumer's level recorded in `need`)
CircOperand circ_row(const tfhe_hip_circuit *c, uint32_t w, int L, std::map<uint32_t, int> &need) {
  const CircExp e = circ_expand(c, w);
  if (circ_plain(e)) return {e.t[0].first, false};
  auto it = need.find(w);
  if (it == need.end() || it->second > L) need[w] = L;
  return {w, true};
}

CircDecision circ_decide(const tfhe_hip_circuit *c, const CircNode &n, std::map<uint32_t, int> &need) {
  CircDecision d;
  const int L = n.level;
  if (n.kind == CN_MUX) return d;  // (rows resolved by the caller)
  uint32_t ca, cb, cc;
  if (n.kind == CN_GATE) {
    GatePrep gp;
    gate_prep(n.op, gp);
    ca = gp.ca, cb = gp.cb, cc = gp.cconst;
  } else {
    ca = n.ca, cb = n.cb, cc = n.cc;
  }
  const CircExp ea = circ_expand(c, n.a);
  const CircExp eb = cb ? circ_expand(c, n.b) : CircExp();
  if (n.kind == CN_GATE && circ_plain(ea) && (!cb || circ_plain(eb))) {
    d.kind = CL_GATE;
    d.code = n.op;
    d.x = {ea.t[0].first, false};
    d.y = {cb ? eb.t[0].first : ea.t[0].first, false};
    return d;
  }
  CircExp comb;
  circ_axpy(comb, ca, ea);
  if (cb) circ_axpy(comb, cb, eb);
  comb.k += cc;
  if (comb.t.size() <= 2) {  // fold into the prologue
    const uint32_t w1 = comb.t.size() > 0 ? comb.t[0].first : 0u, c1 = comb.t.size() > 0 ? comb.t[0].second : 0u;
    const uint32_t w2 = comb.t.size() > 1 ? comb.t[1].first : w1, c2 = comb.t.size() > 1 ? comb.t[1].second : 0u;
    if (n.kind == CN_GATE) {  // still one of the gate codes: the level's gate launch
      for (int g = 0; g <= TFHE_HIP_COPY; ++g) {
        GatePrep gp;
        gate_prep(g, gp);
        if (gp.cconst != comb.k) continue;
        if (gp.ca == c1 && gp.cb == c2) {
          d.kind = CL_GATE, d.code = (uint8_t)g, d.x = {w1, false}, d.y = {w2, false};
          return d;
        }
        if (comb.t.size() == 2 && gp.ca == c2 && gp.cb == c1) {
          d.kind = CL_GATE, d.code = (uint8_t)g, d.x = {w2, false}, d.y = {w1, false};
          return d;
        }
      }
    }
    d.kind = CL_LUT;
    d.lut = n.kind == CN_GATE ? kGateTv : n.lut;
    d.ca = c1, d.cb = c2, d.cc = comb.k;
    d.x = {w1, false};
    d.y = {w2, false};
    return d;
  }
  // more than two source wires: materialise the linear operands, the bootstrap keeps its own coefficients
  d.x = circ_row(c, n.a, L, need);
  d.y = cb ? circ_row(c, n.b, L, need) : d.x;
  if (n.kind == CN_GATE) {
    d.kind = CL_GATE;
    d.code = n.op;
  } else {
    d.kind = CL_LUT;
    d.lut = n.lut, d.ca = ca, d.cb = cb, d.cc = cc;
  }
  return d;
}

int circ_compile(tfhe_hip_circuit *c) {
  if (c->compiled) return TFHE_HIP_OK;
  const size_t W = c->nodes.size();
  int depth = 0;
  for (auto &n : c->nodes)
    if (n.kind != CN_INPUT && n.kind != CN_LIN) depth = std::max(depth, n.level);
  std::map<uint32_t, int> need;  // linear node -> earliest level that needs it materialised
  std::vector<CircDecision> dec(W);
  std::vector<std::array<CircOperand, 3>> mux_rows(W);
  for (uint32_t w = 0; w < W; ++w) {
    const CircNode &n = c->nodes[w];
    if (n.kind == CN_PBS && n.fn) dec[w] = dec[n.head];  // a many-LUT node's further functions: its head decides
    else if (n.kind == CN_GATE || n.kind == CN_PBS) dec[w] = circ_decide(c, n, need);
    if (n.kind == CN_MUX)
      mux_rows[w] = {circ_row(c, n.a, n.level, need), circ_row(c, n.b, n.level, need), circ_row(c, n.c, n.level, need)};
  }
  c->slot.assign(W, kNoSlot);
  c->mat_slot.assign(W, kNoSlot);
  c->opnd.assign(W, {});
  c->levels.assign((size_t)depth + 1, CircLevel());
  for (uint32_t w = 0; w < c->n_inputs; ++w) c->slot[w] = w;
  uint64_t next = c->n_inputs;
  c->levels[0].begin = 0;
  c->levels[0].end = c->n_inputs;
  // slots, level by level: [materialised linear nodes | mux halves | gate launch | lut groups]
  std::vector<uint32_t> u1(W, kNoSlot);
  for (int L = 1; L <= depth; ++L) {
    CircLevel &lv = c->levels[(size_t)L];
    lv.begin = (uint32_t)next;
    std::vector<uint32_t> lin, mux, gate;
    std::vector<std::vector<uint32_t>> group;
    std::vector<std::array<uint32_t, 5>> gkey;
    for (auto &kv : need)
      if (kv.second == L) lin.push_back(kv.first);
    for (uint32_t w = 0; w < W; ++w) {
      const CircNode &n = c->nodes[w];
      if (n.level != L || n.kind == CN_INPUT || n.kind == CN_LIN) continue;
      if (n.kind == CN_MUX) {
        mux.push_back(w);
        gate.push_back(w);
      } else if (dec[w].kind == CL_GATE) {
        gate.push_back(w);
      } else if (n.kind == CN_PBS && n.fn) {
        continue;  // placed with its head
      } else {
        const std::array<uint32_t, 5> k = {dec[w].lut, dec[w].ca, dec[w].cb, dec[w].cc, n.kind == CN_PBS ? n.nl : 0u};
        size_t g = 0;
        while (g < gkey.size() && gkey[g] != k) ++g;
        if (g == gkey.size()) {
          gkey.push_back(k);
          group.emplace_back();
        }
        group[g].push_back(w);
      }
    }
    auto row = [&](const CircOperand &o) { return o.mat ? c->mat_slot[o.wire] : c->slot[o.wire]; };
    if (!lin.empty()) {
      CircLaunch l;
      l.kind = CL_LINCOMB;
      l.out_slot = (uint32_t)next;
      l.nodes = (uint32_t)lin.size();
      l.off.push_back(0);
      for (uint32_t x : lin) {
        c->mat_slot[x] = (uint32_t)next++;
        for (auto &t : c->nodes[x].exp.t) {
          l.coef.push_back(t.second);
          l.src.push_back(c->slot[t.first]);
        }
        l.off.push_back((uint32_t)l.src.size());
        l.cst.push_back(c->nodes[x].exp.k);
      }
      lv.launches.push_back(std::move(l));
    }
    if (!mux.empty()) {
      CircLaunch l;
      l.kind = CL_NKS;
      l.out_slot = (uint32_t)next;
      l.nodes = (uint32_t)(2 * mux.size());
      for (int half = 0; half < 2; ++half)
        for (uint32_t w : mux) {
          const auto &r = mux_rows[w];
          if (!half) u1[w] = (uint32_t)next;
          ++next;
          l.sa.push_back(row(r[0]));
          l.sb.push_back(row(r[half ? 2 : 1]));
          l.code.push_back(half ? TFHE_HIP_ANDNY : TFHE_HIP_AND);  // and(not(a), c) = -a + c - 1/8 (gates.rs:172-175)
          c->opnd[w].push_back(row(r[half ? 2 : 1]));
          if (!half) c->opnd[w].insert(c->opnd[w].begin(), row(r[0]));
        }
      lv.launches.push_back(std::move(l));
    }
    if (!gate.empty()) {
      CircLaunch l;
      l.kind = CL_GATE;
      l.out_slot = (uint32_t)next;
      l.nodes = (uint32_t)gate.size();
      for (uint32_t w : gate) {
        c->slot[w] = (uint32_t)next++;
        if (c->nodes[w].kind == CN_MUX) {
          l.sa.push_back(u1[w]);
          l.sb.push_back(u1[w] + (uint32_t)mux.size());
          l.code.push_back(TFHE_HIP_OR);
        } else {
          l.sa.push_back(row(dec[w].x));
          l.sb.push_back(row(dec[w].y));
          l.code.push_back(dec[w].code);
          c->opnd[w] = {l.sa.back(), l.sb.back()};
        }
      }
      lv.launches.push_back(std::move(l));
    }
    for (size_t g = 0; g < group.size(); ++g) {
      CircLaunch l;
      l.kind = CL_LUT;
      l.out_slot = (uint32_t)next;
      l.nodes = (uint32_t)group[g].size();
      l.lut = gkey[g][0], l.ca = gkey[g][1], l.cb = gkey[g][2], l.cc = gkey[g][3], l.n_luts = gkey[g][4];
      const uint64_t base = next;
      for (uint32_t w : group[g]) {
        c->slot[w] = (uint32_t)next++;
        l.sa.push_back(row(dec[w].x));
        l.sb.push_back(row(dec[w].y));
        c->opnd[w] = {l.sa.back()};
        if (l.cb) c->opnd[w].push_back(l.sb.back());
      }
      if (l.n_luts) {  // function j of node q: slot base + j * nodes + q
        next = base + (uint64_t)l.n_luts * l.nodes;
        if (next > 0xFFFFFFFFull) return TFHE_HIP_EINVAL;
        for (uint32_t q = 0; q < l.nodes; ++q)
          for (uint32_t j = 1; j < l.n_luts; ++j) {
            const uint32_t w = group[g][q] + j;  // the head's further functions are the wires right after it
            c->slot[w] = (uint32_t)(base + (uint64_t)j * l.nodes + q);
            c->opnd[w] = c->opnd[group[g][q]];
          }
      }
      lv.launches.push_back(std::move(l));
    }
    lv.end = (uint32_t)next;
    if (next > 0xFFFFFFFFull) return TFHE_HIP_EINVAL;
  }
  c->slots = (uint32_t)next;
  c->compiled = true;
  return TFHE_HIP_OK;
}

// ---- device plan ---------------------------------------------------------------------------------------------
// Builds (context id, B)'s index arrays, gate codes, lincomb CSR and test vectors in two blobs on the current device.
int circ_plan(tfhe_hip_ctx *ctx, tfhe_hip_circuit *c, size_t B, bool pool, std::shared_ptr<CircPlan> &out) {
  std::lock_guard<std::mutex> lk(c->mu);
  CHK(circ_compile(c) == TFHE_HIP_OK ? TFHE_HIP_OK : fail(ctx, TFHE_HIP_EINVAL, "circuit does not compile"));
  if (B == 0 || (uint64_t)c->slots * B >= 0x100000000ull)
    return fail(ctx, TFHE_HIP_EINVAL, "circuit: slots x batch must be below 2^32 (and batch > 0)");
  const auto key = std::make_tuple(ctx->id, B, pool);
  const auto found = c->plans.find(key);
  if (found != c->plans.end()) {
    found->second->last_use = ++c->plan_tick;
    out = found->second;
    return TFHE_HIP_OK;
  }
  std::shared_ptr<CircPlan> p = std::make_shared<CircPlan>();
  p->device = ctx->device;
  p->B = B;
  p->pool = pool;
  std::vector<uint32_t> u;
  std::vector<uint8_t> u8;
  struct Off { size_t ia, ib, code, tv, off, coef, src, cst, ga_off, ga_coef, ga_src, gb_src; };
  std::vector<std::vector<Off>> offs(c->levels.size());
  std::vector<size_t> lut_at(c->luts.size(), (size_t)-1);
  for (size_t L = 1; L < c->levels.size(); ++L)
    for (const CircLaunch &l : c->levels[L].launches) {
      Off o{};
      const size_t count = (size_t)l.nodes * B;
      p->max_count = std::max(p->max_count, count);
      if (l.kind == CL_LINCOMB) {
        o.off = u.size(); u.insert(u.end(), l.off.begin(), l.off.end());
        o.coef = u.size(); u.insert(u.end(), l.coef.begin(), l.coef.end());
        o.src = u.size(); u.insert(u.end(), l.src.begin(), l.src.end());
        o.cst = u.size(); u.insert(u.end(), l.cst.begin(), l.cst.end());
      } else {
        o.ia = u.size();
        for (uint32_t k = 0; k < l.nodes; ++k)
          for (size_t j = 0; j < B; ++j) u.push_back((uint32_t)(l.sa[k] * B + j));
        o.ib = u.size();
        for (uint32_t k = 0; k < l.nodes; ++k)
          for (size_t j = 0; j < B; ++j) u.push_back((uint32_t)(l.sb[k] * B + j));
        o.ga_off = u.size();
        for (uint32_t k = 0; k <= l.nodes; ++k) u.push_back(k);
        o.ga_coef = u.size();
        u.insert(u.end(), l.nodes, 1u);
        o.ga_src = u.size(); u.insert(u.end(), l.sa.begin(), l.sa.end());
        o.gb_src = u.size(); u.insert(u.end(), l.sb.begin(), l.sb.end());
        o.code = u8.size();
        for (uint32_t k = 0; k < l.nodes; ++k) u8.insert(u8.end(), B, l.code.empty() ? (uint8_t)0 : l.code[k]);
        if (l.kind == CL_LUT && l.lut != kGateTv) {
          if (lut_at[l.lut] == (size_t)-1) {
            lut_at[l.lut] = u.size();
            u.insert(u.end(), c->luts[l.lut].begin(), c->luts[l.lut].end());
          }
          o.tv = lut_at[l.lut];
        } else {
          o.tv = (size_t)-1;
        }
      }
      offs[L].push_back(o);
    }
  if (!u.empty()) {
    CHK(alloc_exact(ctx, p->blob, u.size() * 4, "hipMalloc(&p->blob, u.size() * 4)"));
    HIPCHK(ctx, hipMemcpy(p->blob, u.data(), u.size() * 4, hipMemcpyHostToDevice));
  }
  if (!u8.empty()) {
    CHK(alloc_exact(ctx, p->blob8, u8.size(), "hipMalloc(&p->blob8, u8.size())"));
    HIPCHK(ctx, hipMemcpy(p->blob8, u8.data(), u8.size(), hipMemcpyHostToDevice));
  }
  const uint32_t *U = (const uint32_t *)p->blob.p;
  const uint8_t *U8 = (const uint8_t *)p->blob8.p;
  p->lv.resize(c->levels.size());
  for (size_t L = 1; L < c->levels.size(); ++L)
    for (size_t q = 0; q < c->levels[L].launches.size(); ++q) {
      const Off &o = offs[L][q];
      CircDevLaunch d;
      if (c->levels[L].launches[q].kind == CL_LINCOMB) {
        d.off = U + o.off, d.coef = U + o.coef, d.src = U + o.src, d.cst = U + o.cst;
      } else {
        d.ia = U + o.ia, d.ib = U + o.ib, d.code = U8 + o.code;
        d.ga_off = U + o.ga_off, d.ga_coef = U + o.ga_coef, d.ga_src = U + o.ga_src, d.gb_src = U + o.gb_src;
        d.tv = o.tv == (size_t)-1 ? nullptr : U + o.tv;
      }
      p->lv[L].push_back(d);
    }
  while (c->plans.size() >= kCircMaxPlans) {  // bounded: a long-lived circuit run at many batch sizes keeps four
    auto lru = c->plans.begin();
    for (auto it = c->plans.begin(); it != c->plans.end(); ++it)
      if (it->second->last_use < lru->second->last_use) lru = it;
    c->plans.erase(lru);  // freed when the last run holding it returns
  }
  p->last_use = ++c->plan_tick;
  c->plans[key] = p;
  out = p;
  return TFHE_HIP_OK;
}

unsigned circ_grid(size_t total) { return (unsigned)std::min<size_t>((total + 255) / 256, (size_t)1 << 20); }

int circ_lincomb_launch(tfhe_hip_ctx *ctx, hipStream_t s, const uint32_t *wires, const uint32_t *off, const uint32_t *coef,
                        const uint32_t *src, const uint32_t *cst, size_t B, uint32_t *out, size_t nodes) {
  const uint32_t w = (uint32_t)ctx->P.n + 1;
  const size_t total = nodes * B * w;
  if (!total) return TFHE_HIP_OK;
  hipLaunchKernelGGL(k_circuit_lincomb, dim3(circ_grid(total)), dim3(256), 0, s, wires, off, coef, src, cst, (uint32_t)B, w,
                     out, total);
  HIPCHK(ctx, hipGetLastError());
  return TFHE_HIP_OK;
}

// the whole circuit on one context, every operand gathered in the blind rotation's prologue (mutex held)
int circ_run_locked(tfhe_hip_ctx *ctx, tfhe_hip_circuit *c, const CircPlan *p, uint32_t *wires, hipStream_t s) {
  const size_t B = p->B, w = (size_t)ctx->P.n + 1;
  for (size_t L = 1; L < c->levels.size(); ++L)
    for (size_t q = 0; q < c->levels[L].launches.size(); ++q) {
      const CircLaunch &l = c->levels[L].launches[q];
      const CircDevLaunch &d = p->lv[L][q];
      const size_t count = (size_t)l.nodes * B;
      uint32_t *out = wires + (size_t)l.out_slot * B * w;
      if (l.kind == CL_LINCOMB) {
        CHK(circ_lincomb_launch(ctx, s, wires, d.off, d.coef, d.src, d.cst, B, out, l.nodes));
      } else if (l.kind == CL_NKS) {
        CHK(run_bootstrap(ctx, s, {.in_a = wires, .in_b = wires, .gp = kCodesPrep, .count = count, .gate_codes = d.code, .idx_a = d.ia, .idx_b = d.ib},
                          out, false));
      } else {
        // gates: per-ciphertext codes; lut groups: one (ca, cb, cconst) for the launch (many-LUT groups: k extractions
        // per blind rotation, [k][count] rows through one key switch)
        const bool gate = l.kind == CL_GATE;
        const GatePrep gp = gate ? kCodesPrep : GatePrep{l.ca, l.cb, l.cc};
        CHK(run_bootstrap(ctx, s,
                          {.in_a = wires, .in_b = gp.cb ? wires : nullptr, .gp = gp, .testvec = d.tv, .count = count,
                           .gate_codes = gate ? d.code : nullptr, .idx_a = d.ia, .idx_b = gp.cb ? d.ib : nullptr,
                           .lut_shift = l.n_luts ? lut_shift_of((int)l.n_luts) : 0},
                          out, true));
      }
    }
  return TFHE_HIP_OK;
}

// out[k][B][n+1] = wire out_wires[k] in the caller's numbering (mutex held)
int circ_gather_locked(tfhe_hip_ctx *ctx, tfhe_hip_circuit *c, CircPlan *p, const uint32_t *wires, const uint32_t *out_wires,
                       size_t n_out, uint32_t *out, hipStream_t s) {
  if (!n_out) return TFHE_HIP_OK;
  for (size_t k = 0; k < n_out; ++k)
    if (!circ_wire_ok(c, out_wires[k])) return fail(ctx, TFHE_HIP_EINVAL, "circuit: no such wire");
  if (p->gather_key.size() != n_out || !std::equal(p->gather_key.begin(), p->gather_key.end(), out_wires)) {
    std::vector<uint32_t> off{0}, coef, src, cst;
    for (size_t k = 0; k < n_out; ++k) {
      const CircExp e = circ_expand(c, out_wires[k]);
      for (auto &t : e.t) {
        coef.push_back(t.second);
        src.push_back(c->slot[t.first]);
      }
      off.push_back((uint32_t)src.size());
      cst.push_back(e.k);
    }
    std::vector<uint32_t> u(off);
    p->gather_offs = {0, u.size()};
    u.insert(u.end(), coef.begin(), coef.end());
    p->gather_offs.push_back(u.size());
    u.insert(u.end(), src.begin(), src.end());
    p->gather_offs.push_back(u.size());
    u.insert(u.end(), cst.begin(), cst.end());
    if (p->gather_recorded) HIPCHK(ctx, hipEventSynchronize(p->gather_done));  // the last gather, on whatever stream
    CHK(ensure(ctx, p->gather, u.size() * 4));
    HIPCHK(ctx, hipMemcpy(p->gather.p, u.data(), u.size() * 4, hipMemcpyHostToDevice));
    p->gather_key.assign(out_wires, out_wires + n_out);
  }
  const uint32_t *G = (const uint32_t *)p->gather.p;
  CHK(circ_lincomb_launch(ctx, s, wires, G + p->gather_offs[0], G + p->gather_offs[1], G + p->gather_offs[2],
                          G + p->gather_offs[3], p->B, out, n_out));
  if (!p->gather_done) CHK(hip_rc(ctx, {p->gather_done.create(hipEventDisableTiming), "hipEventCreateWithFlags(&p->gather_done, hipEventDisableTiming)"}));
  HIPCHK(ctx, hipEventRecord(p->gather_done, circ_rt_stream(s)));
  p->gather_recorded = true;
  return TFHE_HIP_OK;
}

int circ_check_ctx(tfhe_hip_ctx *ctx, tfhe_hip_circuit *c) {
  if (!c) return fail(ctx, TFHE_HIP_EINVAL, "circuit is NULL");
  return TFHE_HIP_OK;
}

// ---- pool: one level at a time, operands gathered into staging on the home member, the pool's own _dev calls ----
// (each takes the pool's mutex itself; the home member's lock is taken around what runs on it alone).  The plan's
// run_mu is held by the caller from circ_pool_begin to circ_pool_end: it is always taken before any context's or the
// pool's lock, never while one is held.
int circ_pool_plan(tfhe_hip_ctx *hctx, tfhe_hip_circuit *c, size_t B, std::shared_ptr<CircPlan> &out) {
  ENTER(hctx);
  CHK(circ_check_ctx(hctx, c));
  return circ_plan(hctx, c, B, true, out);
}
// staging, the previous run's end (it may have been enqueued on another stream), the inputs (run_mu held)
int circ_pool_begin(tfhe_hip_ctx *hctx, tfhe_hip_circuit *c, CircPlan *p, const uint32_t *inputs, uint32_t *wires,
                    hipStream_t s) {
  ENTER(hctx);
  const size_t w = (size_t)hctx->P.n + 1, bytes = p->max_count * w * 4;
  if (p->run_recorded) HIPCHK(hctx, hipStreamWaitEvent(circ_rt_stream(s), p->run_done, 0));
  CHK(ensure(hctx, p->stage_a, bytes));
  CHK(ensure(hctx, p->stage_b, bytes));
  if (inputs && inputs != wires)
    HIPCHK(hctx, hipMemcpyAsync(wires, inputs, (size_t)c->n_inputs * p->B * w * 4, hipMemcpyDeviceToDevice, s));
  return TFHE_HIP_OK;
}
// the run's last work on the home stream (every member's shard is back there): the next run waits for it (run_mu held)
int circ_pool_end(tfhe_hip_ctx *hctx, CircPlan *p, hipStream_t s) {
  ENTER(hctx);
  if (!p->run_done) CHK(hip_rc(hctx, {p->run_done.create(hipEventDisableTiming), "hipEventCreateWithFlags(&p->run_done, hipEventDisableTiming)"}));
  HIPCHK(hctx, hipEventRecord(p->run_done, circ_rt_stream(s)));
  p->run_recorded = true;
  return TFHE_HIP_OK;
}
int circ_pool_lincomb(tfhe_hip_ctx *hctx, const uint32_t *wires, const uint32_t *off, const uint32_t *coef,
                      const uint32_t *src, const uint32_t *cst, size_t B, uint32_t *out, size_t nodes, hipStream_t s) {
  ENTER(hctx);
  return circ_lincomb_launch(hctx, s, wires, off, coef, src, cst, B, out, nodes);
}

// every level of the circuit through the pool (run_mu of `p` held by the caller)
int circ_pool_levels(tfhe_hip_pool *pool, int home, tfhe_hip_circuit *c, CircPlan *p, const uint32_t *inputs, uint32_t *wires,
                     hipStream_t s) {
  tfhe_hip_ctx *h = pool->ctxs[(size_t)home];
  tfhe_hip_ctx *hb = h->parent ? h->parent : h;
  const size_t B = p->B, w = (size_t)h->P.n + 1;
  int rc = circ_pool_begin(h, c, p, inputs, wires, s);
  if (rc != TFHE_HIP_OK) return pool_fail(pool, rc, std::string("home member: ") + tfhe_hip_last_error(hb));
  uint32_t *sa = (uint32_t *)p->stage_a.p, *sb = (uint32_t *)p->stage_b.p;
  for (size_t L = 1; L < c->levels.size(); ++L)
    for (size_t q = 0; q < c->levels[L].launches.size(); ++q) {
      const CircLaunch &l = c->levels[L].launches[q];
      const CircDevLaunch &d = p->lv[L][q];
      const size_t count = (size_t)l.nodes * B;
      uint32_t *out = wires + (size_t)l.out_slot * B * w;
      if (l.kind == CL_LINCOMB) {
        rc = circ_pool_lincomb(h, wires, d.off, d.coef, d.src, d.cst, B, out, l.nodes, s);
        if (rc != TFHE_HIP_OK) return pool_fail(pool, rc, std::string("home member: ") + tfhe_hip_last_error(hb));
        continue;
      }
      const bool two = l.kind != CL_LUT || l.cb;
      rc = circ_pool_lincomb(h, wires, d.ga_off, d.ga_coef, d.ga_src, nullptr, B, sa, l.nodes, s);
      if (rc == TFHE_HIP_OK && two) rc = circ_pool_lincomb(h, wires, d.ga_off, d.ga_coef, d.gb_src, nullptr, B, sb, l.nodes, s);
      if (rc != TFHE_HIP_OK) return pool_fail(pool, rc, std::string("home member: ") + tfhe_hip_last_error(hb));
      if (l.kind == CL_NKS) rc = tfhe_hip_pool_batch_gates_mixed_nks_dev(pool, home, d.code, sa, sb, out, count, s);
      else if (l.kind == CL_GATE) rc = tfhe_hip_pool_batch_gates_mixed_dev(pool, home, d.code, sa, sb, out, count, s);
      else if (l.n_luts)
        rc = tfhe_hip_pool_batch_lincomb_bootstrap_many_dev(pool, home, l.ca, sa, l.cb, two ? sb : nullptr, l.cc, d.tv, 0,
                                                            (int)l.n_luts, 1, out, count, s);
      else
        rc = tfhe_hip_pool_batch_lincomb_bootstrap_dev(pool, home, l.ca, sa, l.cb, two ? sb : nullptr, l.cc, d.tv, 0, 1, out,
                                                       count, s);
      if (rc != TFHE_HIP_OK) return rc;
    }
  rc = circ_pool_end(h, p, s);
  if (rc != TFHE_HIP_OK) return pool_fail(pool, rc, std::string("home member: ") + tfhe_hip_last_error(hb));
  return TFHE_HIP_OK;
}

int circ_run_pool_dev(tfhe_hip_pool *pool, int home, tfhe_hip_circuit *c, const uint32_t *inputs, uint32_t *wires, size_t B,
                      void *stream) {
  if (!pool || home < 0 || (size_t)home >= pool->ctxs.size()) return TFHE_HIP_EINVAL;
  tfhe_hip_ctx *h = pool->ctxs[(size_t)home];
  tfhe_hip_ctx *hb = h->parent ? h->parent : h;
  if (!c || !wires) return pool_fail(pool, TFHE_HIP_EINVAL, "circuit or store is NULL");
  std::shared_ptr<CircPlan> p;
  const int rc = circ_pool_plan(h, c, B, p);
  if (rc != TFHE_HIP_OK) return pool_fail(pool, rc, std::string("home member: ") + tfhe_hip_last_error(hb));
  std::lock_guard<std::mutex> run(p->run_mu);
  return circ_pool_levels(pool, home, c, p.get(), inputs, wires, pick(hb, stream));
}

}  // namespace

extern "C" {

int tfhe_hip_circuit_create(uint32_t n_inputs, tfhe_hip_circuit **out) {
  if (!out || n_inputs == 0 || n_inputs >= 0x7FFFFFFFu) return TFHE_HIP_EINVAL;
  tfhe_hip_circuit *c = new (std::nothrow) tfhe_hip_circuit();
  if (!c) return TFHE_HIP_ENOMEM;
  c->n_inputs = n_inputs;
  c->nodes.resize(n_inputs);
  *out = c;
  return TFHE_HIP_OK;
}

void tfhe_hip_circuit_destroy(tfhe_hip_circuit *circ) { delete circ; }

#define CIRC_ADD(circ)                          \
  if (!(circ)) return TFHE_HIP_EINVAL;          \
  std::lock_guard<std::mutex> clk_((circ)->mu); \
  if ((circ)->compiled) return TFHE_HIP_EINVAL

int tfhe_hip_circuit_add_gate(tfhe_hip_circuit *circ, int gate, uint32_t a, uint32_t b, uint32_t *wire) {
  CIRC_ADD(circ);
  if (gate < 0 || gate > TFHE_HIP_COPY || !circ_wire_ok(circ, a) || !circ_wire_ok(circ, b)) return TFHE_HIP_EINVAL;
  CircNode n;
  n.kind = CN_GATE, n.op = (uint8_t)gate, n.a = a, n.b = b;
  n.level = 1 + std::max(circ->nodes[a].level, gate == TFHE_HIP_COPY ? 0 : circ->nodes[b].level);
  return circ_push(circ, std::move(n), wire);
}

int tfhe_hip_circuit_add_mux(tfhe_hip_circuit *circ, uint32_t a, uint32_t b, uint32_t c, uint32_t *wire) {
  CIRC_ADD(circ);
  if (!circ_wire_ok(circ, a) || !circ_wire_ok(circ, b) || !circ_wire_ok(circ, c)) return TFHE_HIP_EINVAL;
  CircNode n;
  n.kind = CN_MUX, n.a = a, n.b = b, n.c = c;
  n.level = 1 + std::max({circ->nodes[a].level, circ->nodes[b].level, circ->nodes[c].level});
  return circ_push(circ, std::move(n), wire);
}

int tfhe_hip_circuit_add_lut(tfhe_hip_circuit *circ, const uint32_t *testvec, uint32_t *lut) {
  CIRC_ADD(circ);
  if (!testvec) return TFHE_HIP_EINVAL;
  circ->luts.emplace_back(testvec, testvec + 2 * kN);
  if (lut) *lut = (uint32_t)circ->luts.size() - 1;
  return TFHE_HIP_OK;
}

int tfhe_hip_circuit_add_pbs(tfhe_hip_circuit *circ, uint32_t ca, uint32_t a, uint32_t cb, uint32_t b, uint32_t cconst,
                             uint32_t lut, uint32_t *wire) {
  CIRC_ADD(circ);
  if (!circ_wire_ok(circ, a) || (cb && !circ_wire_ok(circ, b)) || lut >= circ->luts.size()) return TFHE_HIP_EINVAL;
  CircNode n;
  n.kind = CN_PBS, n.a = a, n.b = cb ? b : a, n.ca = ca, n.cb = cb, n.cc = cconst, n.lut = lut;
  n.level = 1 + std::max(circ->nodes[a].level, cb ? circ->nodes[b].level : 0);
  return circ_push(circ, std::move(n), wire);
}

// k consecutive wires wires[0..k-1]: function j of the packed table `lut` (generate_many_lookup_table) of one bootstrap
int tfhe_hip_circuit_add_pbs_many(tfhe_hip_circuit *circ, uint32_t ca, uint32_t a, uint32_t cb, uint32_t b,
                                  uint32_t cconst, uint32_t lut, int n_luts, uint32_t *wires) {
  CIRC_ADD(circ);
  if (lut_shift_of(n_luts) < 0 || !wires) return TFHE_HIP_EINVAL;
  if (!circ_wire_ok(circ, a) || (cb && !circ_wire_ok(circ, b)) || lut >= circ->luts.size()) return TFHE_HIP_EINVAL;
  if (circ->nodes.size() + (size_t)n_luts >= 0x7FFFFFFFu) return TFHE_HIP_EINVAL;
  CircNode n;
  n.kind = CN_PBS, n.a = a, n.b = cb ? b : a, n.ca = ca, n.cb = cb, n.cc = cconst, n.lut = lut;
  n.level = 1 + std::max(circ->nodes[a].level, cb ? circ->nodes[b].level : 0);
  n.nl = (uint8_t)n_luts;
  n.head = (uint32_t)circ->nodes.size();
  for (int j = 0; j < n_luts; ++j) {
    n.fn = (uint8_t)j;
    CHK(circ_push(circ, n, wires + j));
  }
  return TFHE_HIP_OK;
}

int tfhe_hip_circuit_add_lincomb(tfhe_hip_circuit *circ, const uint32_t *coefs, const uint32_t *wires, size_t n_terms,
                                 uint32_t cconst, uint32_t *wire) {
  CIRC_ADD(circ);
  if (n_terms && (!coefs || !wires)) return TFHE_HIP_EINVAL;
  CircNode n;
  n.kind = CN_LIN;
  n.exp.k = cconst;
  for (size_t i = 0; i < n_terms; ++i) {
    if (!circ_wire_ok(circ, wires[i])) return TFHE_HIP_EINVAL;
    circ_axpy(n.exp, coefs[i], circ_expand(circ, wires[i]));
  }
  n.level = circ_level_of(circ, n.exp);
  return circ_push(circ, std::move(n), wire);
}

int tfhe_hip_circuit_add_not(tfhe_hip_circuit *circ, uint32_t a, uint32_t *wire) {  // gates.rs:202-204: -a
  const uint32_t neg = 0xFFFFFFFFu;
  return tfhe_hip_circuit_add_lincomb(circ, &neg, &a, 1, 0u, wire);
}

int tfhe_hip_circuit_add_constant(tfhe_hip_circuit *circ, int value, uint32_t *wire) {
  // gates.rs:212-219: b = mu = 1/8 for true, 1 - mu (wrapping: quirk Q6) for false
  return tfhe_hip_circuit_add_lincomb(circ, nullptr, nullptr, 0, value ? 0x20000000u : 0xE0000001u, wire);
}
#undef CIRC_ADD

int tfhe_hip_circuit_compile(tfhe_hip_circuit *circ) {
  if (!circ) return TFHE_HIP_EINVAL;
  std::lock_guard<std::mutex> lk(circ->mu);
  return circ_compile(circ);
}

int tfhe_hip_circuit_describe(tfhe_hip_circuit *circ, uint32_t *levels, size_t cap, size_t *n_levels) {
  if (!circ) return TFHE_HIP_EINVAL;
  std::lock_guard<std::mutex> lk(circ->mu);
  CHK(circ_compile(circ));
  if (n_levels) *n_levels = circ->levels.size();
  if (!levels) return TFHE_HIP_OK;
  for (size_t L = 0; L < circ->levels.size() && L < cap; ++L) {
    uint32_t *q = levels + L * TFHE_HIP_CIRCUIT_LEVEL_WORDS;
    std::fill(q, q + TFHE_HIP_CIRCUIT_LEVEL_WORDS, 0u);
    q[0] = circ->levels[L].begin;
    q[1] = circ->levels[L].end;
    for (const CircLaunch &l : circ->levels[L].launches) {
      q[2 + 2 * l.kind] += 1;
      q[3 + 2 * l.kind] += l.nodes;
    }
  }
  return TFHE_HIP_OK;
}

int tfhe_hip_circuit_slots(tfhe_hip_circuit *circ, uint32_t *slots) {
  if (!circ || !slots) return TFHE_HIP_EINVAL;
  std::lock_guard<std::mutex> lk(circ->mu);
  CHK(circ_compile(circ));
  *slots = circ->slots;
  return TFHE_HIP_OK;
}

int tfhe_hip_circuit_wire_slot(tfhe_hip_circuit *circ, uint32_t wire, uint32_t *slot) {
  if (!circ || !slot) return TFHE_HIP_EINVAL;
  std::lock_guard<std::mutex> lk(circ->mu);
  CHK(circ_compile(circ));
  if (!circ_wire_ok(circ, wire)) return TFHE_HIP_EINVAL;
  *slot = circ->slot[wire];
  return TFHE_HIP_OK;
}

int tfhe_hip_circuit_operand_slots(tfhe_hip_circuit *circ, uint32_t wire, uint32_t *slots, uint32_t *n) {
  if (!circ || !slots || !n) return TFHE_HIP_EINVAL;
  std::lock_guard<std::mutex> lk(circ->mu);
  CHK(circ_compile(circ));
  if (!circ_wire_ok(circ, wire)) return TFHE_HIP_EINVAL;
  const auto &o = circ->opnd[wire];
  *n = (uint32_t)o.size();
  std::copy(o.begin(), o.end(), slots);
  return TFHE_HIP_OK;
}

int tfhe_hip_circuit_run_dev(tfhe_hip_ctx *ctx, tfhe_hip_circuit *circ, const uint32_t *inputs, uint32_t *wires, size_t batch,
                             void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(circ_check_ctx(ctx, circ));
  CHK(need_key(ctx));
  if (!wires) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  std::shared_ptr<CircPlan> p;
  CHK(circ_plan(ctx, circ, batch, false, p));
  const hipStream_t s = pick(ctx, stream);
  if (inputs && inputs != wires)
    HIPCHK(ctx, hipMemcpyAsync(wires, inputs, (size_t)circ->n_inputs * batch * (ctx->P.n + 1) * 4, hipMemcpyDeviceToDevice, s));
  return circ_run_locked(ctx, circ, p.get(), wires, s);
}

int tfhe_hip_circuit_gather_dev(tfhe_hip_ctx *ctx, tfhe_hip_circuit *circ, const uint32_t *wires, size_t batch,
                                const uint32_t *out_wires, size_t n_out, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(circ_check_ctx(ctx, circ));
  if (n_out && (!wires || !out_wires || !out)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  std::shared_ptr<CircPlan> p;
  CHK(circ_plan(ctx, circ, batch, false, p));
  return circ_gather_locked(ctx, circ, p.get(), wires, out_wires, n_out, out, pick(ctx, stream));
}

int tfhe_hip_circuit_run(tfhe_hip_ctx *ctx, tfhe_hip_circuit *circ, const uint32_t *inputs, size_t batch,
                         const uint32_t *out_wires, size_t n_out, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(circ_check_ctx(ctx, circ));
  CHK(need_key(ctx));
  if (!inputs || (n_out && (!out_wires || !out))) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  std::shared_ptr<CircPlan> p;
  CHK(circ_plan(ctx, circ, batch, false, p));
  const size_t w = (size_t)ctx->P.n + 1, row = batch * w * 4;
  CHK(ensure(ctx, p->store, (size_t)circ->slots * row));
  uint32_t *wires = (uint32_t *)p->store.p;
  HIPCHK(ctx, hipMemcpyAsync(wires, inputs, (size_t)circ->n_inputs * row, hipMemcpyHostToDevice, ctx->stream));
  CHK(circ_run_locked(ctx, circ, p.get(), wires, ctx->stream));
  if (!n_out) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TFHE_HIP_OK;
  }
  CHK(ensure(ctx, ctx->out.dev, n_out * row));
  CHK(circ_gather_locked(ctx, circ, p.get(), wires, out_wires, n_out, (uint32_t *)ctx->out.dev.p, ctx->stream));
  return to_host(ctx, out, ctx->out, n_out * row);
}

int tfhe_hip_circuit_run_pool_dev(tfhe_hip_pool *pool, int home, tfhe_hip_circuit *circ, const uint32_t *inputs,
                                  uint32_t *wires, size_t batch, void *stream) {
  return circ_run_pool_dev(pool, home, circ, inputs, wires, batch, stream);
}

int tfhe_hip_circuit_gather_pool_dev(tfhe_hip_pool *pool, int home, tfhe_hip_circuit *circ, const uint32_t *wires, size_t batch,
                                     const uint32_t *out_wires, size_t n_out, uint32_t *out, void *stream) {
  if (!pool || home < 0 || (size_t)home >= pool->ctxs.size()) return TFHE_HIP_EINVAL;
  return tfhe_hip_circuit_gather_dev(pool->ctxs[(size_t)home], circ, wires, batch, out_wires, n_out, out, stream);
}

int tfhe_hip_circuit_run_pool(tfhe_hip_pool *pool, tfhe_hip_circuit *circ, const uint32_t *inputs, size_t batch,
                              const uint32_t *out_wires, size_t n_out, uint32_t *out) {
  if (!pool || pool->ctxs.empty()) return TFHE_HIP_EINVAL;
  if (!circ || !inputs || (n_out && (!out_wires || !out))) return pool_fail(pool, TFHE_HIP_EINVAL, "null pointer");
  tfhe_hip_ctx *h = pool->ctxs[0];
  tfhe_hip_ctx *hb = h->parent ? h->parent : h;
  const size_t w = (size_t)h->P.n + 1, row = batch * w * 4;
  std::shared_ptr<CircPlan> p;  // member 0's pool plan: its store, staging and gather, all under run_mu
  int rc = circ_pool_plan(h, circ, batch, p);
  if (rc != TFHE_HIP_OK) return pool_fail(pool, rc, std::string("home member: ") + tfhe_hip_last_error(hb));
  std::lock_guard<std::mutex> run(p->run_mu);
  uint32_t *wires = nullptr;
  {  // the store and the inputs on member 0, after the plan's previous run
    tfhe_hip_ctx *ctx = h;
    ENTER(ctx);
    if (p->run_recorded) HIPCHK(ctx, hipStreamWaitEvent(circ_rt_stream(ctx->stream), p->run_done, 0));
    CHK(ensure(ctx, p->store, (size_t)circ->slots * row));
    wires = (uint32_t *)p->store.p;
    HIPCHK(ctx, hipMemcpyAsync(wires, inputs, (size_t)circ->n_inputs * row, hipMemcpyHostToDevice, ctx->stream));
  }
  CHK(circ_pool_levels(pool, 0, circ, p.get(), nullptr, wires, hb->stream));
  tfhe_hip_ctx *ctx = h;
  ENTER(ctx);
  if (!n_out) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return TFHE_HIP_OK;
  }
  CHK(ensure(ctx, ctx->out.dev, n_out * row));
  CHK(circ_gather_locked(ctx, circ, p.get(), wires, out_wires, n_out, (uint32_t *)ctx->out.dev.p, ctx->stream));
  return to_host(ctx, out, ctx->out, n_out * row);
}

}  // extern "C"
