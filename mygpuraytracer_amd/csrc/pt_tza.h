// pt_tza.h -- host only, no hip* call: an Open Image Denoise 1.4.x weight blob (TZA, format version 2) read into the plan of the RT
// filter's U-Net (pt_nn.hip runs it; the public side and the definition are include/mi355x_pathtracer.h, "network denoiser").
//
// The blob is hostile input: every read is checked against the blob's end, offset + size never wraps, and a tensor's element count is
// formed with a checked multiply.  What is refused comes back as a message that names the tensor; nothing is thrown.
//
// The topology is fixed (OIDN's UNetFilter): enc_conv0, enc_conv1, pool, enc_conv2, pool, enc_conv3, pool, enc_conv4, pool, enc_conv5a,
// enc_conv5b, then four times {upsample, concat with the skip, dec_conv<l>a, dec_conv<l>b}, then dec_conv0.  The skips are pool3, pool2,
// pool1 and the network's input; the upsampled tensor comes first in the channel order.  Channel counts are the blob's.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

struct PtTzaTensor {
    std::string name, layout;             // layout: "x" or "oihw"
    std::vector<uint32_t> dims;
    char type = 'f';                      // 'f' float32, 'h' float16
    uint64_t offset = 0, count = 0;       // where the data begins in the blob; elements
    const uint8_t *data = nullptr;
    // element i as a float (h: converted exactly)
    float at(uint64_t i) const {
        if (type == 'f') { float v; memcpy(&v, data + 4 * i, 4); return v; }
        uint16_t b; memcpy(&b, data + 2 * i, 2);
        return half_bits_to_float(b);
    }
    static float half_bits_to_float(uint16_t b) {
        const uint32_t sign = (uint32_t)(b & 0x8000u) << 16, e = (b >> 10) & 31u, m = b & 1023u;
        uint32_t u;
        if (e == 31) u = sign | 0x7f800000u | (m << 13);
        else if (e) u = sign | ((e + 112u) << 23) | (m << 13);
        else if (!m) u = sign;
        else {                                                       // a subnormal half: m * 2^-24, normal as a float
            uint32_t mm = m, ee = 113;
            while (!(mm & 1024u)) { mm <<= 1; ee--; }
            u = sign | (ee << 23) | ((mm & 1023u) << 13);
        }
        float v; memcpy(&v, &u, 4);
        return v;
    }
};

// One convolution of the plan.  src0 / src1: the layers (indices into PtNnPlan::layers) whose output it reads, -1 = the network's
// input, -2 = none; src0 is upsampled when `upsample`.  cin0 + cin1 = the blob's Cin.
struct PtNnLayer {
    const char *name;
    int cin0 = 0, cin1 = 0, cout = 0;
    int level = 0;                        // its output (before `pool`) is the padded frame >> level
    bool relu = true, pool = false, upsample = false;
    int src0 = -2, src1 = -2;
    const PtTzaTensor *weight = nullptr, *bias = nullptr;
};

constexpr int PT_NN_LAYERS = 16;
constexpr int PT_NN_MAX_CHANNELS = 256;

struct PtNnPlan {
    std::vector<PtTzaTensor> tensors;     // in the table's order
    PtNnLayer layers[PT_NN_LAYERS];
    int ic = 0;
};

namespace pt_tza_detail {
struct Cursor {
    const uint8_t *base; size_t size, pos;
    bool take(void *dst, size_t n) {
        if (pos > size || size - pos < n) return false;
        memcpy(dst, base + pos, n); pos += n;
        return true;
    }
    template <class T> bool read(T &v) { return take(&v, sizeof(T)); }
};
}  // namespace pt_tza_detail

// The blob's table.  False: `err` says what is wrong (with the tensor's name once that is known).
inline bool pt_tza_parse(const void *blob, size_t bytes, std::vector<PtTzaTensor> &out, std::string &err) {
    using pt_tza_detail::Cursor;
    out.clear();
    if (!blob) { err = "the weight blob is NULL"; return false; }
    Cursor c{static_cast<const uint8_t *>(blob), bytes, 0};
    const char *const SHORT = "the weight blob ends inside its ";
    uint16_t magic; uint8_t major, minor; uint64_t table;
    if (!c.read(magic) || !c.read(major) || !c.read(minor) || !c.read(table)) { err = std::string(SHORT) + "header"; return false; }
    if (magic != 0x41D7) { err = "not a TZA weight blob (magic is not 0x41D7)"; return false; }
    if (major != 2) { err = "unsupported TZA version " + std::to_string((int)major) + " (2 is read)"; return false; }
    if (table > bytes) { err = "the weight blob's table offset lies beyond its end"; return false; }
    c.pos = (size_t)table;
    uint32_t count;
    if (!c.read(count)) { err = std::string(SHORT) + "table"; return false; }
    for (uint32_t i = 0; i < count; i++) {
        PtTzaTensor t;
        const std::string nth = "tensor " + std::to_string(i);
        uint16_t len;
        if (!c.read(len)) { err = std::string(SHORT) + "table (" + nth + ")"; return false; }
        if (c.size - c.pos < len) { err = "the name of " + nth + " runs past the weight blob's end"; return false; }
        t.name.assign(reinterpret_cast<const char *>(c.base + c.pos), len);
        c.pos += len;
        const std::string who = "tensor '" + t.name + "'";
        uint8_t ndims;
        if (!c.read(ndims)) { err = std::string(SHORT) + "table (" + who + ")"; return false; }
        t.dims.resize(ndims);
        for (auto &d : t.dims)
            if (!c.read(d)) { err = std::string(SHORT) + "table (" + who + ")"; return false; }
        if (c.size - c.pos < ndims) { err = std::string(SHORT) + "table (" + who + ")"; return false; }
        t.layout.assign(reinterpret_cast<const char *>(c.base + c.pos), ndims);
        c.pos += ndims;
        if (t.layout != "x" && t.layout != "oihw") { err = who + ": layout is neither x nor oihw"; return false; }
        char type;
        if (!c.read(type) || !c.read(t.offset)) { err = std::string(SHORT) + "table (" + who + ")"; return false; }
        if (type != 'f' && type != 'h') { err = who + ": data type '" + std::string(1, type) + "' is neither f nor h"; return false; }
        t.type = type;
        uint64_t n = 1;
        for (const uint32_t d : t.dims) {
            if (d == 0) { err = who + ": a dimension is 0"; return false; }
            if (__builtin_mul_overflow(n, (uint64_t)d, &n)) { err = who + ": the product of its dimensions overflows"; return false; }
        }
        uint64_t size;
        if (__builtin_mul_overflow(n, (uint64_t)(type == 'f' ? 4 : 2), &size)) { err = who + ": the product of its dimensions overflows"; return false; }
        if (t.offset > bytes || bytes - t.offset < size) { err = who + ": its data runs past the weight blob's end"; return false; }
        t.count = n;
        t.data = c.base + t.offset;
        out.push_back(std::move(t));
    }
    return true;
}

// The plan: the table, then the graph with the blob's channel counts checked along it.
inline bool pt_nn_plan(const void *blob, size_t bytes, PtNnPlan &p, std::string &err) {
    if (!pt_tza_parse(blob, bytes, p.tensors, err)) return false;
    // name, level, pool, upsample, src0, src1 (-1 the input, -2 none)
    static const struct { const char *name; int level; bool pool, up; int s0, s1; } G[PT_NN_LAYERS] = {
        {"enc_conv0", 0, false, false, -1, -2}, {"enc_conv1", 0, true, false, 0, -2},  {"enc_conv2", 1, true, false, 1, -2},
        {"enc_conv3", 2, true, false, 2, -2},   {"enc_conv4", 3, true, false, 3, -2},  {"enc_conv5a", 4, false, false, 4, -2},
        {"enc_conv5b", 4, false, false, 5, -2}, {"dec_conv4a", 3, false, true, 6, 3},  {"dec_conv4b", 3, false, false, 7, -2},
        {"dec_conv3a", 2, false, true, 8, 2},   {"dec_conv3b", 2, false, false, 9, -2}, {"dec_conv2a", 1, false, true, 10, 1},
        {"dec_conv2b", 1, false, false, 11, -2}, {"dec_conv1a", 0, false, true, 12, -1}, {"dec_conv1b", 0, false, false, 13, -2},
        {"dec_conv0", 0, false, false, 14, -2}};
    auto find = [&](const std::string &name) -> const PtTzaTensor * {
        for (const auto &t : p.tensors) if (t.name == name) return &t;
        return nullptr;
    };
    for (int i = 0; i < PT_NN_LAYERS; i++) {
        PtNnLayer &L = p.layers[i];
        L.name = G[i].name; L.level = G[i].level; L.pool = G[i].pool; L.upsample = G[i].up; L.src0 = G[i].s0; L.src1 = G[i].s1;
        L.relu = i != PT_NN_LAYERS - 1;
        const std::string wn = std::string(L.name) + ".weight", bn = std::string(L.name) + ".bias";
        L.weight = find(wn); L.bias = find(bn);
        if (!L.weight) { err = "tensor '" + wn + "' is missing from the weight blob"; return false; }
        if (!L.bias) { err = "tensor '" + bn + "' is missing from the weight blob"; return false; }
        const auto &wd = L.weight->dims;
        if (wd.size() != 4 || L.weight->layout != "oihw") { err = "tensor '" + wn + "' must have rank 4 (oihw)"; return false; }
        if (wd[2] != 3 || wd[3] != 3) { err = "tensor '" + wn + "' must be [Cout, Cin, 3, 3]"; return false; }
        if (wd[0] > (uint32_t)PT_NN_MAX_CHANNELS || wd[1] > 2u * PT_NN_MAX_CHANNELS) { err = "tensor '" + wn + "': more than 256 channels"; return false; }
        if (L.bias->dims.size() != 1 || L.bias->layout != "x") { err = "tensor '" + bn + "' must have rank 1 (x)"; return false; }
        if (L.bias->dims[0] != wd[0]) { err = "tensor '" + bn + "' must be [Cout] = [" + std::to_string(wd[0]) + "]"; return false; }
        L.cout = (int)wd[0];
        const int cin = (int)wd[1];
        if (i == 0) {
            if (cin != 3 && cin != 6 && cin != 9) { err = "tensor '" + wn + "': the network takes 3, 6 or 9 input channels, not " + std::to_string(cin); return false; }
            p.ic = cin;
        }
        L.cin0 = L.src0 == -1 ? p.ic : p.layers[L.src0].cout;
        L.cin1 = L.src1 == -2 ? 0 : L.src1 == -1 ? p.ic : p.layers[L.src1].cout;
        if (cin != L.cin0 + L.cin1) {
            err = "tensor '" + wn + "': Cin is " + std::to_string(cin) + ", the graph feeds it " + std::to_string(L.cin0 + L.cin1);
            return false;
        }
        if (L.cin0 > PT_NN_MAX_CHANNELS || L.cin1 > PT_NN_MAX_CHANNELS) { err = "tensor '" + wn + "': more than 256 channels"; return false; }
    }
    if (p.layers[PT_NN_LAYERS - 1].cout != 3) { err = "tensor 'dec_conv0.weight': the network gives 3 output channels, not " + std::to_string(p.layers[PT_NN_LAYERS - 1].cout); return false; }
    return true;
}
