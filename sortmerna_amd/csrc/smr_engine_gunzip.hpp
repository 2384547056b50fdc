// smr_engine_gunzip.hpp -- host side of the DEFLATE decoder (smr_gunzip.hpp; included by smr_engine.hip): gunz_device, which inflates a gzip
// file that lies in host memory into a device buffer, and smr_gunzip_batch, the same with the bytes copied back (a building block and the
// tests' seam).  smr_reads_upload_fastx* under SMR_FASTX_INFLATE (smr_engine_fastx.hpp) inflate into the text buffer of their stream.
//
// The host's share: the candidates of k_gunz_find are sorted; the counting pass runs from every one of them to the next; the pieces are
// stitched -- a piece is confirmed when a confirmed piece ended exactly at its start; an end that hits no start becomes a new piece, counted
// in a further round --; confirmed pieces less than `grain` compressed bytes apart are joined to tasks, which get their output offsets, are
// decoded again to symbols, the windows are made in task order, the symbols resolved; the CRC-32 of the units are joined with zlib's crc32_combine and compared, with ISIZE, to every trailer.
// Whatever does not settle that way -- GUNZ_ROUNDS rounds used up, a decode error in a confirmed task, a mismatch -- is answered "not on the
// device": the caller then runs the host inflate (smr::gunzip_bytes), whose answer or refusal is the call's.
#include <zlib.h>

#include <map>

namespace {
#define GUNZ_ROUNDS 8u
// grain 0: tasks 64 KiB of compressed bytes apart in a file of GUNZ_GRAIN_MANY candidates or more, else a task per candidate (a small file
// has too few of them to fill the device: profiles/gunzip_cost.log)
#define GUNZ_GRAIN_DEFAULT 65536u
#define GUNZ_GRAIN_MANY 4096u
#define GUNZ_GRAIN_MAX (16u << 20)       // a task of the writing pass stays well inside GUNZ_PIECE_BITS
#define GUNZ_SPARSE_BYTES (16u << 20)    // compressed bytes per candidate above which the file is the host's

// why a call took the host path (smr_gunzip_info)
enum { GUNZ_WHY_NONE = 0, GUNZ_WHY_NOT_TAKEN, GUNZ_WHY_CANDIDATES, GUNZ_WHY_ROUNDS, GUNZ_WHY_DECODE, GUNZ_WHY_DISTANCE, GUNZ_WHY_CHECK, GUNZ_WHY_TRUNCATED,
       GUNZ_WHY_TRAILING, GUNZ_WHY_HEADER_CRC };

struct GunzHostTask { uint64_t start; uint32_t kind; bool extra, counted; uint64_t stop; GunzRes res; };

// the report of a call: under err_m, like smr_fastx_info's
void gunz_report(smr_ctx* c, GunzScratch& S, uint64_t why, uint64_t rounds, uint64_t cand, uint64_t tasks, uint64_t members, const uint64_t blocks[3], uint64_t n, uint64_t plain,
                 std::vector<uint64_t>&& starts) {
  double ms[6];
  S.clk.copy_to(ms);
  std::lock_guard<std::mutex> l_(c->err_m);
  c->gunz_info[0] = (why ? 1u : 0u) | (why << 8) | (rounds << 16);
  c->gunz_info[1] = cand; c->gunz_info[2] = tasks; c->gunz_info[3] = members;
  c->gunz_info[4] = blocks[0] | (blocks[1] << 32); c->gunz_info[5] = blocks[2];
  c->gunz_info[6] = n; c->gunz_info[7] = plain;
  for (int k = 0; k < 6; k++) c->gunz_ms[k] = why ? 0.0 : ms[k];
  c->gunz_tasks = std::move(starts);
}

// The n bytes at h_gz, a gzip file -> `plain` bytes at the start of `out` (reserved for ((plain + 15) & ~15) + 64 bytes, the layout of a text
// buffer of fastx_upload).  *device = false: not settled on the device, `out` holds nothing of use and the caller inflates on the host.
// limit != 0: text of `limit` bytes or more is of no use to the caller: *plain says how much there is, *device = false, and the writing pass
// with its allocations (three bytes per byte of text) does not run.
int gunz_device(smr_ctx* c, GunzScratch& S, hipStream_t st, const uint8_t* h_gz, uint64_t n, uint64_t grain, DevBuf<uint8_t>& out, uint64_t* plain, bool* device, uint64_t limit = 0) {
  *device = false; *plain = 0;
  const uint64_t none[3] = {0, 0, 0};
  auto host = [&](uint64_t why, uint64_t rounds = 0, uint64_t cand = 0, uint64_t tasks = 0) { gunz_report(c, S, why, rounds, cand, tasks, 0, none, n, 0, {}); return SMR_OK; };
  if (n < 18u || n >= (1ull << 38) || h_gz[0] != 0x1Fu || h_gz[1] != 0x8Bu || h_gz[2] != 8u || (h_gz[3] & 0xE0u)) return host(GUNZ_WHY_NOT_TAKEN);
  const uint64_t nbits = n * 8u;
  int rc;
  if ((rc = S.clk.begin(c))) return rc;
  // ---- the bytes, padded with zeros for gunz_peek
  const size_t words = (size_t)(n / 4u) + 8u;
  const uint32_t cap = (uint32_t)std::min<uint64_t>(n / 32u + 1024u, 0x7FFFFFFFu);
  if ((rc = S.in.reserve(c, words)) || (rc = S.cand.reserve(c, cap)) || (rc = S.n_cand.reserve(c, 1))) return rc;
  if ((rc = S.clk.mark(c, 0, st))) return rc;
  HIPCHK(c, hipMemsetAsync((uint8_t*)S.in.get() + (n & ~3ull), 0, 32, st));
  HIPCHK(c, hipMemcpyAsync(S.in, h_gz, (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(S.n_cand, 0, 4, st));
  if ((rc = S.clk.mark(c, 1, st))) return rc;
  // ---- candidates
  launch_on(st, k_gunz_find, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, (const uint32_t*)S.in, (unsigned long long)n, (unsigned long long*)S.cand, cap, (uint32_t*)S.n_cand);
  HIPCHK(c, hipGetLastError());
  if ((rc = S.clk.mark(c, 2, st))) return rc;
  uint32_t n_cand = 0;
  HIPCHK(c, hipMemcpyAsync(&n_cand, S.n_cand, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  S.clk.set(0, 0, 1);
  S.clk.set(1, 1, 2);
  if (n_cand > cap) return host(GUNZ_WHY_CANDIDATES, 0, n_cand);
  std::vector<unsigned long long> cand(n_cand);
  if (n_cand) HIPCHK(c, hipMemcpyAsync(cand.data(), S.cand, (size_t)n_cand * 8u, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  std::sort(cand.begin(), cand.end());
  if (cand.empty() || cand[0] != GUNZ_KIND_MEMBER) return host(GUNZ_WHY_NOT_TAKEN, 0, n_cand);
  // a piece is decoded by ONE wave: a file with next to no candidates (stored or fixed blocks only, another compressor's long blocks) is
  // serial work, which a host core does faster.  k_gunz_decode itself gives up on a piece of more than GUNZ_PIECE_BITS.
  if (n / n_cand > GUNZ_SPARSE_BYTES) return host(GUNZ_WHY_NOT_TAKEN, 0, n_cand);
  grain = std::min<uint64_t>(grain, GUNZ_GRAIN_MAX);
  // ---- the counting pass starts at EVERY candidate and runs to the next one: a false candidate among them is never confirmed and costs
  // nothing, and the pass is as parallel as the file allows; `grain` joins the confirmed pieces to the tasks of the writing pass below
  if (grain == 0) grain = n_cand >= GUNZ_GRAIN_MANY ? GUNZ_GRAIN_DEFAULT : 1u;
  std::vector<GunzHostTask> T;
  std::map<uint64_t, uint32_t> at;                      // start bit * 2 + kind -> piece
  for (uint64_t key : cand) {
    GunzHostTask t = {}; t.start = key >> 1; t.kind = (uint32_t)(key & 1u);
    at[key] = (uint32_t)T.size(); T.push_back(t);
  }
  auto stop_of = [&](uint64_t start) { auto it = at.lower_bound((start + 1u) * 2u); return it == at.end() ? nbits : it->first >> 1; };
  for (auto& t : T) t.stop = stop_of(t.start);
  // ---- the counting pass, in rounds
  std::vector<uint32_t> chain, fresh(T.size());
  for (uint32_t i = 0; i < T.size(); i++) fresh[i] = i;
  uint32_t cur = 0, rounds = 0;
  uint64_t member_before = 0;                           // bytes of the member cur starts in that lie in front of cur
  bool done = false;
  while (!done) {
    if (rounds == GUNZ_ROUNDS) return host(GUNZ_WHY_ROUNDS, rounds, n_cand, T.size());
    rounds++;
    const uint32_t m = (uint32_t)fresh.size();
    std::vector<GunzTask> dt(m);
    for (uint32_t k = 0; k < m; k++) { const GunzHostTask& t = T[fresh[k]]; dt[k].start = t.start; dt[k].stop = t.stop; dt[k].out_off = 0; dt[k].out_cap = 0; dt[k].kind = t.kind; dt[k].pad = 0; }
    if ((rc = S.tasks.reserve(c, m)) || (rc = S.res.reserve(c, m))) return rc;
    HIPCHK(c, hipMemcpyAsync(S.tasks, dt.data(), (size_t)m * sizeof(GunzTask), hipMemcpyHostToDevice, st));
    if ((rc = S.clk.mark(c, 3, st))) return rc;
    launch_on(st, k_gunz_decode<0>, dim3(m), dim3(64), 0, (const uint32_t*)S.in, (unsigned long long)n, (const GunzTask*)S.tasks, (GunzRes*)S.res, (uint16_t*)nullptr);
    HIPCHK(c, hipGetLastError());
    if ((rc = S.clk.mark(c, 4, st))) return rc;
    std::vector<GunzRes> dr(m);
    HIPCHK(c, hipMemcpyAsync(dr.data(), S.res, (size_t)m * sizeof(GunzRes), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    S.clk.add(2, 3, 4);
    for (uint32_t k = 0; k < m; k++) { T[fresh[k]].res = dr[k]; T[fresh[k]].counted = true; }
    fresh.clear();
    // stitch from cur on
    for (;;) {
      const GunzRes& r = T[cur].res;
      if (r.err) return host(r.err == GUNZ_ERR_TRUNC ? GUNZ_WHY_TRUNCATED : r.err == GUNZ_ERR_MAGIC ? GUNZ_WHY_TRAILING : r.err == GUNZ_ERR_DIST ? GUNZ_WHY_DISTANCE : r.err == GUNZ_ERR_LONG ? GUNZ_WHY_NOT_TAKEN : GUNZ_WHY_DECODE,
                             rounds, n_cand, T.size());
      if (r.maxback > member_before) return host(GUNZ_WHY_DISTANCE, rounds, n_cand, T.size());
      member_before = r.n_mem ? r.out_len - r.mem[r.n_mem - 1u].out_rel : member_before + r.out_len;
      chain.push_back(cur);
      if (r.end_kind == GUNZ_KIND_END) { done = true; break; }
      const uint64_t key = r.end * 2u + (r.end_kind == GUNZ_KIND_MEMBER ? 1u : 0u);
      auto it = at.find(key);
      if (it == at.end()) {                             // a false or missing candidate: a task of the next round
        GunzHostTask t = {}; t.start = r.end; t.kind = (uint32_t)(key & 1u); t.extra = true; t.stop = stop_of(r.end);
        it = at.emplace(key, (uint32_t)T.size()).first; T.push_back(t);
      }
      cur = it->second;
      if (!T[cur].counted) { fresh.push_back(cur); break; }
    }
  }
  // ---- the confirmed pieces: members, header CRCs; pieces less than `grain` bytes apart are one task of the writing pass (which passes
  // fewer than GUNZ_MAXM member boundaries, unless it is one piece)
  struct Member { uint64_t end; uint32_t crc, isize; };
  std::vector<Member> members;
  std::vector<GunzTask> dt;
  std::vector<uint64_t> starts, ends;
  uint32_t task_mem = 0;
  uint64_t total = 0, blocks[3] = {0, 0, 0};
  auto header_ok = [&](uint64_t b, uint64_t e) {        // FHCRC: the low 16 bits of the CRC-32 of the header in front of it
    if (!(h_gz[b + 3u] & 2u)) return true;
    const uint32_t want = (uint32_t)h_gz[e - 2u] | ((uint32_t)h_gz[e - 1u] << 8);
    return (uint32_t)(crc32(0L, h_gz + b, (uInt)(e - 2u - b)) & 0xFFFFu) == want;
  };
  for (uint32_t i = 0; i < chain.size(); i++) {
    const GunzHostTask& t = T[chain[i]];
    const GunzRes& r = t.res;
    if (dt.empty() || grain <= 1u || t.start - dt.back().start >= grain * 8u || task_mem + r.n_mem >= GUNZ_MAXM) {
      GunzTask d; d.start = t.start; d.stop = nbits; d.out_off = total; d.out_cap = 0; d.kind = t.kind; d.pad = 0;
      if (!dt.empty()) dt.back().stop = t.start;
      dt.push_back(d); starts.push_back((t.start << 2) | (t.extra ? 2u : 0u) | t.kind); ends.push_back(0);
      task_mem = 0;
    }
    dt.back().out_cap += r.out_len; ends.back() = r.end; task_mem += r.n_mem;
    if (t.kind == GUNZ_KIND_MEMBER && !header_ok(r.hdr_start, r.hdr_end)) return host(GUNZ_WHY_HEADER_CRC, rounds, n_cand, chain.size());
    for (uint32_t k = 0; k < r.n_mem; k++) {
      members.push_back({total + r.mem[k].out_rel, r.mem[k].crc, r.mem[k].isize});
      if (r.mem[k].hdr_end && !header_ok(r.mem[k].hdr_start, r.mem[k].hdr_end)) return host(GUNZ_WHY_HEADER_CRC, rounds, n_cand, chain.size());
    }
    for (int k = 0; k < 3; k++) blocks[k] += r.blocks[k];
    total += r.out_len;
  }
  const uint32_t nt = (uint32_t)dt.size();
  if (limit && total >= limit) { gunz_report(c, S, GUNZ_WHY_NOT_TAKEN, rounds, n_cand, nt, members.size(), blocks, n, total, {}); *plain = total; return SMR_OK; }
  // units: no unit crosses a task's end, a member's end or GUNZ_UNIT bytes
  std::vector<GunzUnit> units;
  {
    size_t mi = 0;
    for (uint32_t i = 0; i < nt; i++) {
      uint64_t o = dt[i].out_off;
      const uint64_t e = o + dt[i].out_cap;
      while (o < e) {
        while (mi < members.size() && members[mi].end <= o) mi++;
        uint64_t len = std::min<uint64_t>(e - o, GUNZ_UNIT);
        if (mi < members.size()) len = std::min(len, members[mi].end - o);
        units.push_back({o, (uint32_t)len, i});
        o += len;
      }
    }
  }
  if (units.size() >= 0x7FFFFFFFull) return host(GUNZ_WHY_NOT_TAKEN, rounds, n_cand, nt);
  const uint32_t nu = (uint32_t)units.size();
  if ((rc = gz_crc_table(c, st))) return rc;
  if ((rc = S.tasks.reserve(c, nt)) || (rc = S.res.reserve(c, nt)) || (rc = S.sym.reserve(c, (size_t)total)) || (rc = S.win.reserve(c, (size_t)nt * GUNZ_WIN)) ||
      (rc = S.units.reserve(c, nu)) || (rc = S.crc.reserve(c, nu)) || (rc = out.reserve(c, (size_t)(((total + 15u) & ~15ull) + 64u)))) return rc;
  HIPCHK(c, hipMemcpyAsync(S.tasks, dt.data(), (size_t)nt * sizeof(GunzTask), hipMemcpyHostToDevice, st));
  if (nu) HIPCHK(c, hipMemcpyAsync(S.units, units.data(), (size_t)nu * sizeof(GunzUnit), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(S.win, 0, GUNZ_WIN, st));
  if ((rc = S.clk.mark(c, 5, st))) return rc;
  launch_on(st, k_gunz_decode<1>, dim3(nt), dim3(64), 0, (const uint32_t*)S.in, (unsigned long long)n, (const GunzTask*)S.tasks, (GunzRes*)S.res, (uint16_t*)S.sym);
  if ((rc = S.clk.mark(c, 6, st))) return rc;
  launch_on(st, k_gunz_window, dim3(1), dim3(1024), 0, (const GunzTask*)S.tasks, nt, (const uint16_t*)S.sym, (uint8_t*)S.win);
  if ((rc = S.clk.mark(c, 7, st))) return rc;
  if (nu) launch_on(st, k_gunz_resolve, dim3(nu), dim3(GZ_WIN), 0, (const GunzUnit*)S.units, (const uint16_t*)S.sym, (const uint8_t*)S.win, (const uint32_t*)c->gz.crc_tab, (uint8_t*)out,
                    (uint32_t*)S.crc);
  HIPCHK(c, hipGetLastError());
  if ((rc = S.clk.mark(c, 3, st))) return rc;          // (the counting rounds are over: their first event serves again)
  std::vector<GunzRes> wr(nt);
  std::vector<uint32_t> crc(nu);
  HIPCHK(c, hipMemcpyAsync(wr.data(), S.res, (size_t)nt * sizeof(GunzRes), hipMemcpyDeviceToHost, st));
  if (nu) HIPCHK(c, hipMemcpyAsync(crc.data(), S.crc, (size_t)nu * 4u, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  S.clk.set(3, 5, 6); S.clk.set(4, 6, 7); S.clk.set(5, 7, 3);
  for (uint32_t i = 0; i < nt; i++) if (wr[i].err || wr[i].out_len != dt[i].out_cap || wr[i].end != ends[i]) return host(GUNZ_WHY_DECODE, rounds, n_cand, nt);
  // ---- CRC-32 and ISIZE of every member
  {
    size_t ui = 0;
    uint64_t begin = 0;
    for (const Member& m : members) {
      uLong sum = crc32(0L, Z_NULL, 0);
      for (; ui < nu && units[ui].off < m.end; ui++) sum = crc32_combine(sum, crc[ui], (z_off_t)units[ui].len);
      if ((uint32_t)sum != m.crc || (uint32_t)(m.end - begin) != m.isize) return host(GUNZ_WHY_CHECK, rounds, n_cand, nt);
      begin = m.end;
    }
  }
  gunz_report(c, S, GUNZ_WHY_NONE, rounds, n_cand, nt, members.size(), blocks, n, total, std::move(starts));
  *plain = total; *device = true;
  return SMR_OK;
}
}  // namespace

extern "C" int smr_gunzip_batch(smr_ctx* c, const uint8_t* gz, uint64_t n, uint64_t grain, uint8_t* plain, uint64_t cap, uint64_t* need) {
  if (!c || !need || (!gz && n)) return SMR_ERR_ARG;
  *need = 0;
  HIPCHK(c, hipSetDevice(c->device));
  GunzScratch& S = c->gunz[0];
  uint64_t total = 0; bool device = false;
  int rc = gunz_device(c, S, c->stream, gz, n, grain, S.out, &total, &device);
  if (rc) return rc;
  std::vector<char> own;
  if (!device) {
    std::string why;
    if (!smr::gunzip_bytes("smr_gunzip_batch", gz, (size_t)n, own, why)) { set_err(c, why); return SMR_ERR_IO; }
    total = own.size();
    std::lock_guard<std::mutex> l_(c->err_m);
    c->gunz_info[7] = total;
  }
  *need = total;
  if (!plain) return SMR_OK;
  if (cap < total) { set_err(c, "smr_gunzip_batch: the file inflates to " + std::to_string(total) + " bytes, the buffer has " + std::to_string(cap)); return SMR_ERR_CAPACITY; }
  if (!device) { if (total) memcpy(plain, own.data(), (size_t)total); return SMR_OK; }
  if (total) HIPCHK(c, hipMemcpyAsync(plain, S.out, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SMR_OK;
}
extern "C" int smr_gunzip_info(const smr_ctx* c, uint64_t info[8]) {
  if (!c || !info) return SMR_ERR_ARG;
  std::lock_guard<std::mutex> l_(const_cast<smr_ctx*>(c)->err_m);
  for (int k = 0; k < 8; k++) info[k] = c->gunz_info[k];
  return SMR_OK;
}
extern "C" int smr_gunzip_times(const smr_ctx* c, double ms[6]) {
  if (!c || !ms) return SMR_ERR_ARG;
  std::lock_guard<std::mutex> l_(const_cast<smr_ctx*>(c)->err_m);
  for (int k = 0; k < 6; k++) ms[k] = c->gunz_ms[k];
  return SMR_OK;
}
extern "C" int smr_gunzip_tasks(const smr_ctx* c, uint64_t* starts, uint64_t cap, uint64_t* count) {
  if (!c || !count) return SMR_ERR_ARG;
  std::lock_guard<std::mutex> l_(const_cast<smr_ctx*>(c)->err_m);
  *count = c->gunz_tasks.size();
  if (starts) for (uint64_t k = 0; k < std::min<uint64_t>(cap, *count); k++) starts[k] = c->gunz_tasks[k];
  return SMR_OK;
}
