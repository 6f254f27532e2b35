// Checkpoint and restart of the host driver (include/artemis_driver.h: artemis_sim_save / _restore /
// _checkpoint_describe).  Plain C++ like the rest of the driver; the device is reached only through the copies the
// state already uses (checkpoint_hooks.hpp).
//
// A checkpoint is a directory with one part file per writing rank, part-00000.bin ...  Layout of a part (native byte
// order, refused on a machine of the other one):
//
//   fixed header, 64 bytes   magic "ARTMSCKP" | u32 version | u32 byte-order mark | u32 sizeof(Real) | u32 part |
//                            u32 parts | u32 0 | u64 blocks in this part | u64 bytes of the global header |
//                            u64 doubles of n-body rows | u64 payload bytes per block
//   global header            rank 0's part only (see write_global / read_global)
//   directory                per block: i32 level, lx1, lx2, lx3 | u64 offset of its payload in this file | u64 checksum
//                            of that payload
//   n-body rows              this rank's partial particle_force rows [npart][7], then the sums still held in the device
//                            accumulators [npart][7]
//   u64 checksum             of everything above
//   payload                  per block the whole primitive arrays of the current buffer, ghost zones and the pressure slot
//                            included: gas [6 ns][nk][nj][ni], then dust [4 ns][nk][nj][ni].  Blocks narrower than the
//                            ghost width: the same for the other two ping-pong buffers after it (checkpoint_hooks.hpp)
//
// The payload checksum sits with each block's directory entry, so a reader verifies exactly the blocks it loads: every
// rank reads the heads of all parts and the payload of its own blocks only.  Nothing is allocated from a length field
// before that field has been checked against the size of the file it came from.
#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <dirent.h>
#include <array>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>
#include <vector>

#include "artemis_driver.h"
#include "artemis_hip.h"
#include "checkpoint_hooks.hpp"
#include "parameter_input.hpp"

// The identity of the library's sources is informational here: a host that exports the driver's C ABI without it (the
// CPU stand-in of the tests) writes "unknown".
extern "C" const char *artemis_hip_source_sha(void) __attribute__((weak));

namespace {

std::string source_sha() { return artemis_hip_source_sha ? artemis_hip_source_sha() : "unknown"; }

using artemis_ckpt::BlockKey;
using artemis_ckpt::Meta;

const char kMagic[8] = {'A', 'R', 'T', 'M', 'S', 'C', 'K', 'P'};
constexpr uint32_t kVersion = 1, kByteOrder = 0x01020304u;
constexpr uint64_t kFixed = 64, kDirEntry = 32;

// where the last save / restore of this thread spent its time: {total, device copies, checksums, file reads or writes}
thread_local double g_seconds[4] = {0.0, 0.0, 0.0, 0.0};
struct Lap {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double operator()() {
    const auto t1 = std::chrono::steady_clock::now();
    const double s = std::chrono::duration<double>(t1 - t0).count();
    t0 = t1;
    return s;
  }
};

struct Fail : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// 64-bit multiply-xor hash over 8-byte words (the payload is doubles; a tail of < 8 bytes is padded with zeros)
uint64_t checksum(const void *data, size_t n, uint64_t h = 0x9E3779B97F4A7C15ull) {
  const unsigned char *p = static_cast<const unsigned char *>(data);
  size_t q = 0;
  for (; q + 8 <= n; q += 8) {
    uint64_t w;
    std::memcpy(&w, p + q, 8);
    h = (h ^ w) * 0x100000001B3ull;
    h ^= h >> 29;
  }
  if (q < n) {
    uint64_t w = 0;
    std::memcpy(&w, p + q, n - q);
    h = (h ^ w) * 0x100000001B3ull;
    h ^= h >> 29;
  }
  return h ^ static_cast<uint64_t>(n);
}

struct Writer {
  std::vector<unsigned char> b;
  void raw(const void *p, size_t n) {
    const unsigned char *c = static_cast<const unsigned char *>(p);
    b.insert(b.end(), c, c + n);
  }
  template <class T>
  void put(T v) {
    raw(&v, sizeof v);
  }
  void str(const std::string &s) {
    put<uint64_t>(s.size());
    raw(s.data(), s.size());
  }
};

struct Reader {
  const unsigned char *p;
  size_t n, at = 0;
  Reader(const unsigned char *p_, size_t n_) : p(p_), n(n_) {}
  size_t left() const { return n - at; }
  void raw(void *out, size_t k) {
    if (k > left()) throw Fail("the header ends before its fields do");
    std::memcpy(out, p + at, k);
    at += k;
  }
  template <class T>
  T get() {
    T v;
    raw(&v, sizeof v);
    return v;
  }
  std::string str() {
    const uint64_t k = get<uint64_t>();
    if (k > left()) throw Fail("a string of the header is longer than the header");
    std::string s(reinterpret_cast<const char *>(p + at), static_cast<size_t>(k));
    at += static_cast<size_t>(k);
    return s;
  }
};

void write_global(Writer &w, const Meta &m) {
  w.str(source_sha());
  w.str(m.deck);
  w.put<uint64_t>(m.overrides.size());
  for (const std::string &o : m.overrides) w.str(o);
  w.put<double>(m.time), w.put<double>(m.dt);
  w.put<int64_t>(m.ncycle), w.put<int64_t>(m.remeshes), w.put<int64_t>(m.nranks), w.put<int64_t>(m.nblocks_global);
  for (int d = 0; d < 3; ++d) w.put<int32_t>(m.mbnx[d]);
  w.put<int32_t>(m.ni), w.put<int32_t>(m.nj), w.put<int32_t>(m.nk), w.put<int32_t>(m.nghost), w.put<int32_t>(m.ndim);
  w.put<int32_t>(m.ns_gas), w.put<int32_t>(m.ns_dust), w.put<int32_t>(m.coords);
  w.put<int32_t>(m.multilevel), w.put<int32_t>(m.adaptive), w.put<int32_t>(m.npart), w.put<int32_t>(m.nbuf), w.put<int32_t>(m.base);
  w.str(m.integrator);
  w.put<uint64_t>(m.deref_count.size());
  for (const auto &e : m.deref_count)
    for (int q = 0; q < 5; ++q) w.put<int32_t>(e[q]);
}

void read_global(Reader &r, Meta &m, std::string &sha) {
  sha = r.str();
  m.deck = r.str();
  const uint64_t nover = r.get<uint64_t>();
  if (nover > r.left() / 8) throw Fail("the override count of the header exceeds the header");
  for (uint64_t q = 0; q < nover; ++q) m.overrides.push_back(r.str());
  m.time = r.get<double>(), m.dt = r.get<double>();
  m.ncycle = static_cast<long>(r.get<int64_t>()), m.remeshes = static_cast<long>(r.get<int64_t>());
  const int64_t nranks = r.get<int64_t>();
  m.nblocks_global = static_cast<long>(r.get<int64_t>());
  for (int d = 0; d < 3; ++d) m.mbnx[d] = r.get<int32_t>();
  m.ni = r.get<int32_t>(), m.nj = r.get<int32_t>(), m.nk = r.get<int32_t>(), m.nghost = r.get<int32_t>(), m.ndim = r.get<int32_t>();
  m.ns_gas = r.get<int32_t>(), m.ns_dust = r.get<int32_t>(), m.coords = r.get<int32_t>();
  m.multilevel = r.get<int32_t>(), m.adaptive = r.get<int32_t>(), m.npart = r.get<int32_t>();
  m.nbuf = r.get<int32_t>(), m.base = r.get<int32_t>();
  m.integrator = r.str();
  const uint64_t nderef = r.get<uint64_t>();
  if (nderef > r.left() / 20) throw Fail("the derefinement map of the header exceeds the header");
  for (uint64_t q = 0; q < nderef; ++q) {
    std::array<int, 5> e;
    for (int c = 0; c < 5; ++c) e[c] = r.get<int32_t>();
    m.deref_count.push_back(e);
  }
  if (r.left() != 0) throw Fail("the global header is longer than its fields");
  auto in = [](long v, long lo, long hi) { return v >= lo && v <= hi; };
  if (!in(nranks, 1, 1 << 20) || !in(m.ni, 1, 1 << 16) || !in(m.nj, 1, 1 << 16) || !in(m.nk, 1, 1 << 16) || !in(m.ns_gas, 0, 64) ||
      !in(m.ns_dust, 0, 64) || !in(m.nghost, 0, 64) || !in(m.ndim, 1, 3) || !in(m.npart, 0, 1 << 20) || m.nblocks_global < 1 ||
      m.ncycle < 0 || m.remeshes < 0 || (m.nbuf != 1 && m.nbuf != 3) || !in(m.base, 0, 2))
    throw Fail("a field of the global header is out of range");
  m.nranks = static_cast<int>(nranks);
}

uint64_t buffer_bytes(const Meta &m) { // one ping-pong buffer of one block (every factor was range-checked: below 2^61)
  return (6ull * m.ns_gas + 4ull * m.ns_dust) * static_cast<uint64_t>(m.ni) * m.nj * m.nk * sizeof(double);
}
uint64_t payload_bytes(const Meta &m) { return buffer_bytes(m) * static_cast<uint64_t>(m.nbuf); }

std::string part_name(const std::string &dir, long part) {
  char buf[32];
  std::snprintf(buf, sizeof buf, "/part-%05ld.bin", part);
  return dir + buf;
}

struct File { // closes on scope exit
  FILE *f = nullptr;
  std::string name;
  File(const std::string &n, const char *mode) : f(std::fopen(n.c_str(), mode)), name(n) {}
  ~File() {
    if (f) std::fclose(f);
  }
  uint64_t size() const {
    struct stat st;
    if (fstat(fileno(f), &st) != 0 || st.st_size < 0) throw Fail("cannot stat " + name);
    return static_cast<uint64_t>(st.st_size);
  }
  void read_at(uint64_t off, void *out, size_t n) {
    if (fseeko(f, static_cast<off_t>(off), SEEK_SET) != 0 || std::fread(out, 1, n, f) != n)
      throw Fail("truncated part: " + name + " ends before byte " + std::to_string(off + n));
  }
  void write_at(uint64_t off, const void *in, size_t n) {
    if (fseeko(f, static_cast<off_t>(off), SEEK_SET) != 0 || std::fwrite(in, 1, n, f) != n)
      throw Fail("cannot write " + name + ": " + std::strerror(errno));
  }
};

struct Entry {
  BlockKey key;
  uint64_t offset, sum;
};
struct PartHead {
  uint32_t part = 0, parts = 0;
  uint64_t nblocks = 0, global_len = 0, nrows = 0, block_bytes = 0, head_len = 0, file_size = 0;
  std::vector<unsigned char> global;
  std::vector<Entry> dir;
  std::vector<double> rows;
};

// The head of one part, every length checked against the file before anything is sized from it
void read_head(const std::string &name, PartHead &h) {
  File f(name, "rb");
  if (!f.f) throw Fail("missing part: cannot open " + name + " (" + std::strerror(errno) + ")");
  h.file_size = f.size();
  if (h.file_size < kFixed + 8) throw Fail("truncated part: " + name + " is shorter than a part header");
  unsigned char fx[kFixed];
  f.read_at(0, fx, kFixed);
  if (std::memcmp(fx, kMagic, 8) != 0) throw Fail("wrong magic: " + name + " is not a checkpoint part");
  Reader r(fx + 8, kFixed - 8);
  const uint32_t version = r.get<uint32_t>(), bom = r.get<uint32_t>(), real = r.get<uint32_t>();
  if (bom != kByteOrder) throw Fail("wrong byte order: " + name + " was written on a machine of the other byte order");
  if (version != kVersion) throw Fail("wrong version: " + name + " has format version " + std::to_string(version) + ", this build reads " + std::to_string(kVersion));
  if (real != sizeof(double)) throw Fail(name + " holds reals of " + std::to_string(real) + " bytes, this build uses 8");
  h.part = r.get<uint32_t>(), h.parts = r.get<uint32_t>();
  r.get<uint32_t>();
  h.nblocks = r.get<uint64_t>(), h.global_len = r.get<uint64_t>(), h.nrows = r.get<uint64_t>(), h.block_bytes = r.get<uint64_t>();
  const uint64_t fs = h.file_size;
  if (h.global_len > fs || h.nblocks > fs / kDirEntry || h.nrows > fs / 8 || h.block_bytes > fs)
    throw Fail("truncated part: " + name + " is shorter than its header says");
  h.head_len = kFixed + h.global_len + h.nblocks * kDirEntry + h.nrows * 8 + 8; // (each term <= fs < 2^63 / 4)
  if (h.head_len > fs) throw Fail("truncated part: " + name + " is shorter than its header says");
  if (h.parts < 1 || h.parts > (1u << 20) || h.part >= h.parts) throw Fail("bad part numbering in " + name);
  std::vector<unsigned char> head(static_cast<size_t>(h.head_len));
  f.read_at(0, head.data(), head.size());
  uint64_t want;
  std::memcpy(&want, head.data() + head.size() - 8, 8);
  if (checksum(head.data(), head.size() - 8) != want) throw Fail("checksum mismatch in the header of " + name);
  if (h.block_bytes && h.nblocks > (fs - h.head_len) / h.block_bytes) // (a part is written whole: header, then every block)
    throw Fail("truncated part: " + name + " is shorter than its " + std::to_string(h.nblocks) + " blocks");
  const unsigned char *at = head.data() + kFixed;
  h.global.assign(at, at + h.global_len);
  at += h.global_len;
  h.dir.resize(static_cast<size_t>(h.nblocks));
  for (Entry &e : h.dir) {
    int32_t k[4];
    std::memcpy(k, at, 16), std::memcpy(&e.offset, at + 16, 8), std::memcpy(&e.sum, at + 24, 8);
    at += kDirEntry;
    e.key = {k[0], k[1], k[2], k[3]};
    if (e.offset < h.head_len || e.offset > fs || h.block_bytes > fs - e.offset)
      throw Fail("a directory entry of " + name + " points outside the file");
  }
  h.rows.resize(static_cast<size_t>(h.nrows));
  if (h.nrows) std::memcpy(h.rows.data(), at, static_cast<size_t>(h.nrows) * 8);
}

// Everything a reader learns without touching a device: the global header and the directories of all parts
struct Checkpoint {
  Meta meta;
  std::string sha, dir;
  std::vector<PartHead> parts;
  std::map<BlockKey, std::pair<int, size_t>> where; // block -> (part, directory index)
  uint64_t bytes = 0;
};

std::string strip_slashes(const char *path) {
  std::string d = path ? path : "";
  while (d.size() > 1 && d.back() == '/') d.pop_back();
  if (d.empty()) throw Fail("empty checkpoint path");
  return d;
}

void open_checkpoint(const char *path, Checkpoint &c) {
  c.dir = strip_slashes(path);
  struct stat st;
  if (stat(c.dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) throw Fail("no checkpoint directory at " + c.dir);
  c.parts.resize(1);
  read_head(part_name(c.dir, 0), c.parts[0]);
  if (c.parts[0].part != 0 || c.parts[0].global_len == 0) throw Fail(part_name(c.dir, 0) + " does not open with the global header");
  {
    Reader r(c.parts[0].global.data(), c.parts[0].global.size());
    read_global(r, c.meta, c.sha);
  }
  const uint32_t nparts = c.parts[0].parts;
  if (static_cast<long>(nparts) != c.meta.nranks) throw Fail("the part count does not match the writer rank count of the header");
  const uint64_t bb = payload_bytes(c.meta);
  uint64_t total = 0;
  for (uint32_t p = 0; p < nparts; ++p) {
    if (p > 0) {
      c.parts.emplace_back();
      read_head(part_name(c.dir, p), c.parts.back());
    }
    const PartHead &h = c.parts[p];
    if (h.part != p || h.parts != nparts || (p > 0 && h.global_len != 0)) throw Fail("bad part numbering in " + part_name(c.dir, p));
    if (h.block_bytes != bb) throw Fail("the block size of " + part_name(c.dir, p) + " does not match the block shape of the header");
    if (h.nrows != 14ull * c.meta.npart) throw Fail("the n-body rows of " + part_name(c.dir, p) + " do not match the particle count of the header");
    for (size_t q = 0; q < h.dir.size(); ++q)
      if (!c.where.emplace(h.dir[q].key, std::make_pair(static_cast<int>(p), q)).second)
        throw Fail("a block is listed twice in the part directories");
    total += h.nblocks;
    c.bytes += h.file_size;
  }
  if (total != static_cast<uint64_t>(c.meta.nblocks_global)) throw Fail("the part directories do not hold the global block count of the header");
}

// `failed` summed over the ranks (the communicator's allreduce_sum as barrier and vote); > 0 if anybody failed
bool vote(const artemis_comm_t *comm, bool failed) {
  if (!comm || comm->nranks <= 1) return failed;
  double v = failed ? 1.0 : 0.0;
  if (!comm->allreduce_sum || comm->allreduce_sum(comm->ctx, &v, 1)) return true;
  return v > 0.0;
}

// part files and the directory itself; anything else in there is not ours and keeps the directory
void remove_checkpoint_dir(const std::string &dir) {
  DIR *d = opendir(dir.c_str());
  if (!d) {
    if (errno == ENOENT) return;
    throw Fail("cannot open " + dir + ": " + std::strerror(errno));
  }
  std::vector<std::string> names;
  while (struct dirent *e = readdir(d)) {
    const std::string n = e->d_name;
    if (n.size() == 14 && n.compare(0, 5, "part-") == 0 && n.compare(10, 4, ".bin") == 0) names.push_back(n);
  }
  closedir(d);
  for (const std::string &n : names) unlink((dir + "/" + n).c_str());
  if (rmdir(dir.c_str()) != 0) throw Fail("cannot replace " + dir + " (it holds files that are not checkpoint parts): " + std::strerror(errno));
}

void write_part(artemis_sim_t *sim, const Meta &m, const std::vector<double> &rows, const std::string &name) {
  Writer global;
  if (m.rank == 0) write_global(global, m);
  const uint64_t bb = payload_bytes(m), nblocks = m.blocks.size();
  const uint64_t head_len = kFixed + global.b.size() + nblocks * kDirEntry + rows.size() * 8 + 8;
  File f(name, "wb");
  if (!f.f) throw Fail("cannot create " + name + ": " + std::strerror(errno));
  std::vector<double> buf(static_cast<size_t>(bb / sizeof(double)));
  const size_t one = static_cast<size_t>(buffer_bytes(m) / sizeof(double)), gas_n = 6ull * m.ns_gas * m.ni * m.nj * m.nk;
  std::vector<uint64_t> sums(static_cast<size_t>(nblocks));
  Lap lap;
  for (uint64_t b = 0; b < nblocks; ++b) {
    for (int q = 0; q < m.nbuf; ++q) artemis_ckpt::download_block(sim, static_cast<int>(b), q, buf.data() + q * one, buf.data() + q * one + gas_n);
    g_seconds[1] += lap();
    sums[b] = checksum(buf.data(), static_cast<size_t>(bb));
    g_seconds[2] += lap();
    f.write_at(head_len + b * bb, buf.data(), static_cast<size_t>(bb));
    g_seconds[3] += lap();
  }
  Writer w;
  w.raw(kMagic, 8);
  w.put<uint32_t>(kVersion), w.put<uint32_t>(kByteOrder), w.put<uint32_t>(sizeof(double));
  w.put<uint32_t>(static_cast<uint32_t>(m.rank)), w.put<uint32_t>(static_cast<uint32_t>(m.nranks)), w.put<uint32_t>(0);
  w.put<uint64_t>(nblocks), w.put<uint64_t>(global.b.size()), w.put<uint64_t>(rows.size()), w.put<uint64_t>(bb);
  w.raw(global.b.data(), global.b.size());
  for (uint64_t b = 0; b < nblocks; ++b) {
    for (int q = 0; q < 4; ++q) w.put<int32_t>(m.blocks[b][q]);
    w.put<uint64_t>(head_len + b * bb), w.put<uint64_t>(sums[b]);
  }
  w.raw(rows.data(), rows.size() * 8);
  w.put<uint64_t>(checksum(w.b.data(), w.b.size()));
  f.write_at(0, w.b.data(), w.b.size());
  FILE *fp = f.f;
  f.f = nullptr;
  if (std::fflush(fp) != 0 || std::fclose(fp) != 0) throw Fail("cannot write " + name + ": " + std::strerror(errno));
  g_seconds[3] += lap();
}

std::string override_key(const std::string &o) {
  const auto eq = o.find('=');
  std::string k = o.substr(0, eq);
  const auto a = k.find_first_not_of(" \t"), b = k.find_last_not_of(" \t");
  return a == std::string::npos ? std::string() : k.substr(a, b - a + 1);
}

// Keys that fix the shape of what is stored.  An extra override may repeat the stored value, never change it.
const char *const kShapeKeys[] = {"parthenon/meshblock/nx1", "parthenon/meshblock/nx2", "parthenon/meshblock/nx3", "parthenon/mesh/nx1",
                                  "parthenon/mesh/nx2", "parthenon/mesh/nx3", "parthenon/mesh/nghost", "parthenon/mesh/refinement",
                                  "artemis/coordinates", "physics/gas", "physics/dust", "gas/nspecies", "dust/nspecies"};
bool is_shape_key(const std::string &k) {
  for (const char *s : kShapeKeys)
    if (k == s) return true;
  return false;
}

void refuse_shape_overrides(const Meta &m, int nover, const char *const *over) {
  artemis_host::ParameterInput was;
  was.LoadFromString(m.deck);
  for (const std::string &o : m.overrides) was.ApplyOverride(o);
  for (int q = 0; q < nover; ++q) {
    if (!over || !over[q]) throw Fail("null override");
    const std::string o = over[q], k = override_key(o);
    const auto eq = o.find('='), slash = k.rfind('/');
    if (eq == std::string::npos || slash == std::string::npos) throw Fail("bad override: " + o);
    if (!is_shape_key(k)) continue;
    const std::string blk = k.substr(0, slash), key = k.substr(slash + 1);
    if (!was.DoesParameterExist(blk, key)) continue; // (a default of the deck: the restored state is compared below)
    artemis_host::ParameterInput now;
    now.ApplyOverride(o);
    const std::string a = was.GetString(blk, key), b = now.GetString(blk, key);
    char *ea = nullptr, *eb = nullptr;
    const double va = std::strtod(a.c_str(), &ea), vb = std::strtod(b.c_str(), &eb);
    const bool numeric = ea != a.c_str() && eb != b.c_str() && *ea == 0 && *eb == 0;
    if (numeric ? va != vb : a != b)
      throw Fail("restore refuses the override " + k + " = " + b + ": the checkpoint was written with " + a +
                 ", and block shape, ghost zones, species, coordinates and dimensions of a checkpoint are fixed");
  }
}

std::string json_escape(const std::string &s) {
  std::string o;
  char buf[8];
  for (unsigned char c : s) {
    if (c == '"' || c == '\\') o += '\\', o += static_cast<char>(c);
    else if (c == '\n') o += "\\n";
    else if (c == '\t') o += "\\t";
    else if (c == '\r') o += "\\r";
    else if (c < 0x20) std::snprintf(buf, sizeof buf, "\\u%04x", c), o += buf;
    else o += static_cast<char>(c);
  }
  return o;
}

std::string json_double(double v) { // (dt is DBL_MAX at cycle 0: finite, so every value here prints as a JSON number)
  char buf[40];
  std::snprintf(buf, sizeof buf, "%.17g", v);
  return (v == v && v - v == 0.0) ? std::string(buf) : std::string("null");
}

} // namespace

extern "C" {

int artemis_sim_save(artemis_sim_t *sim, const char *path) {
  if (!sim) {
    artemis_ckpt::set_error("null simulation");
    return 1;
  }
  const artemis_comm_t *comm = artemis_ckpt::comm_of(sim);
  Lap total;
  for (double &v : g_seconds) v = 0.0;
  std::string err, dir, tmp;
  Meta m;
  std::vector<double> rows;
  // every rank takes every vote, whatever happened to it before: the votes are collective
  try {
    const std::string dead = artemis_ckpt::dead_reason(sim);
    if (!dead.empty()) throw Fail(dead);
    dir = strip_slashes(path), tmp = dir + ".tmp";
    artemis_ckpt::prepare_save(sim, rows);
    artemis_ckpt::describe(sim, m);
    if (m.rank == 0) {
      remove_checkpoint_dir(tmp);
      if (mkdir(tmp.c_str(), 0777) != 0) throw Fail("cannot create " + tmp + ": " + std::strerror(errno));
    }
  } catch (const std::exception &e) {
    err = e.what();
  }
  bool failed = vote(comm, !err.empty());
  if (!failed) {
    try {
      write_part(sim, m, rows, part_name(tmp, m.rank));
    } catch (const std::exception &e) {
      err = e.what();
    }
    failed = vote(comm, !err.empty());
  }
  if (!failed) {
    try {
      if (m.rank == 0) {
        remove_checkpoint_dir(dir);
        if (rename(tmp.c_str(), dir.c_str()) != 0) throw Fail("cannot rename " + tmp + " to " + dir + ": " + std::strerror(errno));
      }
    } catch (const std::exception &e) {
      err = e.what();
    }
    failed = vote(comm, !err.empty());
  }
  g_seconds[0] = total();
  if (!failed) return 0;
  if (m.rank == 0 && !tmp.empty()) {
    try {
      remove_checkpoint_dir(tmp);
    } catch (const std::exception &) {
    }
  }
  artemis_ckpt::set_error("artemis_sim_save: " + (err.empty() ? std::string("another rank failed") : err));
  return 1;
}

artemis_sim_t *artemis_sim_restore(const char *path, int noverrides, const char *const *overrides, const artemis_comm_t *comm) {
  std::string err;
  Checkpoint c;
  Lap total;
  for (double &v : g_seconds) v = 0.0;
  try {
    open_checkpoint(path, c);
    if (c.sha != source_sha())
      std::fprintf(stderr, "artemis_sim_restore: %s was written by source %s, this library is %s\n", c.dir.c_str(), c.sha.c_str(),
                   source_sha().c_str());
    refuse_shape_overrides(c.meta, noverrides, overrides);
  } catch (const std::exception &e) {
    err = e.what();
  }
  if (vote(comm, !err.empty())) {
    artemis_ckpt::set_error("artemis_sim_restore: " + (err.empty() ? std::string("another rank failed") : err));
    return nullptr;
  }
  artemis_sim_t *sim = nullptr;
  try {
    const Meta &m = c.meta;
    std::vector<std::string> over = m.overrides;
    std::string extra;
    for (int q = 0; q < noverrides; ++q) over.push_back(overrides[q]), extra += (q ? ", " : "") + override_key(overrides[q]);
    std::vector<BlockKey> leaves; // the tree comes from the file: parts in rank order hold the leaves in Z-order
    if (m.multilevel)
      for (const PartHead &h : c.parts)
        for (const Entry &e : h.dir) leaves.push_back(e.key);
    sim = artemis_ckpt::create_on_leaves(m.deck, over, comm, m.multilevel ? &leaves : nullptr);
    Meta now;
    artemis_ckpt::describe(sim, now);
    const char *what = nullptr;
    if (now.mbnx[0] != m.mbnx[0] || now.mbnx[1] != m.mbnx[1] || now.mbnx[2] != m.mbnx[2] || now.ni != m.ni || now.nj != m.nj || now.nk != m.nk)
      what = "the block shape";
    else if (now.nghost != m.nghost) what = "the number of ghost zones";
    else if (now.ns_gas != m.ns_gas || now.ns_dust != m.ns_dust) what = "the species counts";
    else if (now.coords != m.coords) what = "the coordinate system";
    else if (now.ndim != m.ndim) what = "the dimensionality";
    else if (now.multilevel != m.multilevel || now.nblocks_global != m.nblocks_global) what = "the mesh";
    else if (now.npart != m.npart) what = "the n-body particles";
    else if (now.nbuf != m.nbuf) what = "the block shape";
    if (what)
      throw Fail(std::string("restore refuses the overrides (") + (extra.empty() ? "none" : extra) + "): they change " + what + " of the checkpoint");
    const uint64_t bb = payload_bytes(m);
    std::vector<double> buf(static_cast<size_t>(bb / sizeof(double)));
    const size_t one = static_cast<size_t>(buffer_bytes(m) / sizeof(double)), gas_n = 6ull * m.ns_gas * m.ni * m.nj * m.nk;
    std::vector<std::unique_ptr<File>> files(c.parts.size());
    for (size_t b = 0; b < now.blocks.size(); ++b) {
      const auto it = c.where.find(now.blocks[b]);
      if (it == c.where.end()) throw Fail("the restored mesh holds a block the checkpoint does not");
      const int p = it->second.first;
      const Entry &e = c.parts[p].dir[it->second.second];
      if (!files[p]) {
        files[p].reset(new File(part_name(c.dir, p), "rb"));
        if (!files[p]->f) throw Fail("missing part: cannot open " + part_name(c.dir, p));
      }
      Lap lap;
      files[p]->read_at(e.offset, buf.data(), static_cast<size_t>(bb));
      g_seconds[3] += lap();
      if (checksum(buf.data(), static_cast<size_t>(bb)) != e.sum)
        throw Fail("checksum mismatch in the payload of " + part_name(c.dir, p));
      g_seconds[2] += lap();
      for (int q = 0; q < m.nbuf; ++q)
        artemis_ckpt::upload_block(sim, static_cast<int>(b), m.nbuf == 3 ? m.base : 0, q, buf.data() + q * one, buf.data() + q * one + gas_n);
      g_seconds[1] += lap();
    }
    // n-body sums: rank 0 takes the sum of all parts' rows, everybody else starts from zero
    std::vector<double> rows(14 * static_cast<size_t>(m.npart), 0.0);
    if (now.rank == 0)
      for (const PartHead &h : c.parts)
        for (size_t q = 0; q < rows.size(); ++q) rows[q] += h.rows[q];
    Meta put = m; // clock and remesh history of the file; the overrides of this run stay on the handle
    artemis_ckpt::finish_restore(sim, put, rows);
  } catch (const std::exception &e) {
    err = e.what();
  }
  if (vote(comm, !err.empty())) {
    if (sim) artemis_sim_destroy(sim);
    artemis_ckpt::set_error("artemis_sim_restore: " + (err.empty() ? std::string("another rank failed") : err));
    return nullptr;
  }
  g_seconds[0] = total();
  return sim;
}

void artemis_sim_checkpoint_seconds(double *out4) {
  for (int q = 0; q < 4 && out4; ++q) out4[q] = g_seconds[q];
}

int artemis_sim_checkpoint_describe(const char *path, char *json_out, long capacity) {
  std::string j;
  try {
    Checkpoint c;
    open_checkpoint(path, c);
    const Meta &m = c.meta;
    auto num = [](long v) { return std::to_string(v); };
    j = "{\"format_version\": " + num(kVersion) + ", \"sizeof_real\": 8, \"source_sha\": \"" + json_escape(c.sha) + "\"";
    j += ", \"time\": " + json_double(m.time) + ", \"dt\": " + json_double(m.dt) + ", \"ncycle\": " + num(m.ncycle);
    j += ", \"remeshes\": " + num(m.remeshes) + ", \"nranks\": " + num(m.nranks) + ", \"nblocks\": " + num(m.nblocks_global);
    j += ", \"block_shape\": [" + num(m.mbnx[0]) + ", " + num(m.mbnx[1]) + ", " + num(m.mbnx[2]) + "]";
    j += ", \"block_zones\": [" + num(m.ni) + ", " + num(m.nj) + ", " + num(m.nk) + "]";
    j += ", \"nghost\": " + num(m.nghost) + ", \"ndim\": " + num(m.ndim) + ", \"ns_gas\": " + num(m.ns_gas) + ", \"ns_dust\": " + num(m.ns_dust);
    j += ", \"coords\": " + num(m.coords) + ", \"multilevel\": " + (m.multilevel ? "true" : "false") + ", \"adaptive\": " + (m.adaptive ? "true" : "false");
    j += ", \"buffers\": " + num(m.nbuf);
    j += ", \"nparticles\": " + num(m.npart) + ", \"deref_counters\": " + num(static_cast<long>(m.deref_count.size()));
    j += ", \"integrator\": \"" + json_escape(m.integrator) + "\", \"bytes\": " + std::to_string(c.bytes);
    j += ", \"overrides\": [";
    for (size_t q = 0; q < m.overrides.size(); ++q) j += (q ? ", \"" : "\"") + json_escape(m.overrides[q]) + "\"";
    j += "], \"deck\": \"" + json_escape(m.deck) + "\"}";
  } catch (const std::exception &e) {
    artemis_ckpt::set_error(std::string("artemis_sim_checkpoint_describe: ") + e.what());
    return -1;
  }
  if (json_out && capacity > static_cast<long>(j.size())) std::memcpy(json_out, j.c_str(), j.size() + 1);
  return static_cast<int>(j.size());
}

} // extern "C"
