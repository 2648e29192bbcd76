// Baseline-JPEG image ingest on gfx950 (the image read of detect.py:55-58,
// torchvision.io.read_image(path, ImageReadMode.RGB)).
//
// Split by what each side is good at:
//   host    marker parsing + Huffman decoding (inherently sequential per image; one image per host
//           thread) into a compact "packet": per 8x8 block the list of its nonzero coefficients
//           (natural index, value) plus the quantisation tables.  A COCO-size picture has ~10-20 %
//           nonzero coefficients, so the packet is a few hundred KB and crosses PCIe as such;
//   device  dequantisation + islow IDCT of every block of a batch (one wave = 8 blocks, lane = one
//           column in pass 1 and one row in pass 2, the 8x8 tiles through LDS) into component planes,
//           then fancy chroma upsampling + YCbCr->RGB straight into the uint8 [B,3,H,W] batch the
//           detector plan reads (the CLI's input layout), one thread per output pixel pair.
// All arithmetic is the reference decoder's integer arithmetic (csrc/jpeg_core.hpp), so the bytes equal
// the host decoder's (tests/test_jpeg.py on the host checker, tests/test_gpu_jpeg.py on the device).
// Supported: 8-bit baseline / extended sequential Huffman JPEGs (SOF0 / SOF1, 8- or 16-bit quantisation
// tables), 1 (gray) or 3 (YCbCr) components, 4:4:4, 4:2:2 (h2v1) and 4:2:0 (h2v2) sampling, restart
// intervals, one or several scans (interleaved, per component or mixed; a component no scan names decodes
// as zero coefficients).  As in libjpeg, a chroma component whose downsampled width is 2 or less is
// replicated, not filtered (the narrow-image rule, jpeg_core.hpp), and a component's quantisation table is
// latched when the first scan that names it starts: a DQT that redefines the table id later applies only
// to components not yet scanned, and a scan whose component has no table yet is an error.  Anything else
// (progressive, arithmetic coding, 12-bit, CMYK / RGB JPEGs, other samplings) reports "unsupported" and
// the caller decodes that image on the host.
// Reject policy: the packet holds only what the file's own bits say.  libjpeg decodes damaged entropy
// data with a warning (zero bits after a premature marker or end of file, resynchronisation on a missing
// or out-of-sequence RSTn); this decoder does not emulate that, it rejects such a file (< 0 from
// Decoder::run) and the batch path hands it to the host decoder: a scan that consumed bits its data did
// not supply, a restart boundary not followed by the RSTn expected in sequence, an interleaved scan whose
// components are not in frame order, a bad Huffman code.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "kernels.hpp"
#include "jpeg_core.hpp"

namespace edgedet {
namespace jpeg {

constexpr uint32_t PACKET_MAGIC = 0x504a4445u;  // "EDJP"
constexpr int PACKET_VERSION = 1;

// Packet layout (4-byte aligned, little endian): Header, then blocks[nblocks] {start, count} (uint32
// each), then coef[nnz] uint32 = (uint16)value << 16 | natural index.  Blocks are component-major,
// row-major over the component's MCU-padded block grid (bw x bh).
struct Header {
    uint32_t magic;
    int32_t version, H, W, ncomp, hmax, vmax, mcus_x, mcus_y;
    int32_t h[3], v[3], bw[3], bh[3], cw[3], ch[3], block_base[3];
    int32_t nblocks, nnz, off_blocks, off_coef, bytes;
    int16_t quant[3][64];  // natural order
};

// ------------------------------------------------------------------------------------ host decoder
struct Huff {
    // lookahead: for the first 9 bits, (length << 8) | symbol, 0 = longer code
    uint16_t look[512];
    int32_t maxcode[18];
    int32_t valptr[17];
    int32_t mincode[17];
    uint8_t vals[256];
    bool present = false;
};

static bool build_huff(const uint8_t bits[17], const uint8_t* vals, int nvals, Huff& h) {
    int code = 0, k = 0;
    std::memset(h.look, 0, sizeof(h.look));
    std::memcpy(h.vals, vals, (size_t)nvals);
    int huffsize[257], huffcode[257];
    int p = 0;
    for (int l = 1; l <= 16; ++l)
        for (int i = 0; i < bits[l]; ++i) huffsize[p++] = l;
    huffsize[p] = 0;
    const int lastp = p;
    p = 0;
    int si = huffsize[0];
    while (huffsize[p]) {
        while (huffsize[p] == si) {
            huffcode[p++] = code;
            ++code;
        }
        if (code >= (1 << si)) return false;  // bad table
        code <<= 1;
        ++si;
    }
    p = 0;
    for (int l = 1; l <= 16; ++l) {
        if (bits[l]) {
            h.valptr[l] = p;
            h.mincode[l] = huffcode[p];
            p += bits[l];
            h.maxcode[l] = huffcode[p - 1];
        } else {
            h.maxcode[l] = -1;
        }
    }
    h.maxcode[17] = 0x7fffffff;
    for (p = 0; p < lastp; ++p) {
        const int l = huffsize[p];
        if (l <= 9) {
            const int base = huffcode[p] << (9 - l);
            for (int j = 0; j < (1 << (9 - l)); ++j) h.look[base + j] = (uint16_t)((l << 8) | h.vals[p]);
        }
    }
    (void)k;
    h.present = true;
    return true;
}

struct BitReader {
    const uint8_t* d;
    size_t n, pos;
    uint64_t acc = 0;
    int bits = 0;
    bool marker = false;  // hit a marker: feed zeros (libjpeg's behaviour at a premature marker)
    int fed = 0;          // zero bits fed since the last restart, past a marker or the end of the input
    void fill() {
        // fast path: the next 8 bytes hold no 0xFF (no stuffing, no marker): take the whole bytes that fit
        if (!marker && pos + 8 <= n) {
            uint64_t x;
            std::memcpy(&x, d + pos, 8);
            x = __builtin_bswap64(x);
            const uint64_t nx = ~x;
            if (((nx - 0x0101010101010101ull) & ~nx & 0x8080808080808080ull) == 0) {
                const int nb = (64 - bits) >> 3;  // >= 1 (bits <= 56 here)
                acc |= (x >> (64 - 8 * nb)) << (64 - bits - 8 * nb);
                bits += 8 * nb;
                pos += (size_t)nb;
                return;
            }
        }
        while (bits <= 56) {
            uint32_t byte = 0;
            const bool supplied = !marker && pos < n;
            if (supplied) {
                byte = d[pos];
                if (byte == 0xFF) {
                    const uint32_t nx = pos + 1 < n ? d[pos + 1] : 0;
                    if (nx == 0x00) {
                        pos += 2;
                    } else {
                        marker = true;
                        byte = 0;
                    }
                } else {
                    ++pos;
                }
            }
            if ((!supplied || marker) && fed < 128) fed += 8;  // (saturates: the buffer holds 64 bits)
            acc |= (uint64_t)byte << (56 - bits);
            bits += 8;
        }
    }
    uint32_t peek(int k) {
        if (bits < k) fill();
        return (uint32_t)(acc >> (64 - k));
    }
    void skip(int k) {
        acc <<= k;
        bits -= k;
    }
    uint32_t get(int k) {
        if (k == 0) return 0;
        const uint32_t v = peek(k);
        skip(k);
        return v;
    }
    // The fed zeros are the buffer's tail (every byte after the first fed one is fed too), so the
    // decoder consumed bits the data did not supply exactly when fewer bits are left than were fed.
    // The reader's look-ahead into a closing marker feeds zeros as well, but leaves them in the buffer.
    bool overran() const { return bits < fed; }
    // At a restart boundary: discard the partial byte and step past RST<k>, which must be the next
    // marker.  Every byte of a well-formed interval holds at least one coded bit, so the reader has
    // taken them all and stands at the marker (or the fill 0xFF bytes before it).
    bool restart_marker(int k) {
        acc = 0;
        bits = 0;
        fed = 0;
        marker = false;
        while (pos + 1 < n && d[pos] == 0xFF && d[pos + 1] == 0xFF) ++pos;
        if (pos + 1 >= n || d[pos] != 0xFF || d[pos + 1] != 0xD0 + k) return false;
        pos += 2;
        return true;
    }
};

static inline int decode_sym(BitReader& br, const Huff& h) {
    const uint32_t look = h.look[br.peek(9)];
    if (look) {
        br.skip(look >> 8);
        return look & 0xFF;
    }
    int l = 10;
    int32_t code = (int32_t)br.peek(l);
    while (l <= 16 && code > h.maxcode[l]) {
        ++l;
        code = (int32_t)br.peek(l);
    }
    if (l > 16) return -1;
    br.skip(l);
    return h.vals[h.valptr[l] + code - h.mincode[l]];
}

static inline int extend(uint32_t v, int s) { return s == 0 ? 0 : (v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v); }

struct Comp {
    int id, h, v, tq;
};

// Parse + entropy-decode one file into a packet (returns its byte size, 0 = unsupported, < 0 = error)
struct Decoder {
    std::string err;
    int H = 0, W = 0, ncomp = 0, hmax = 1, vmax = 1, restart = 0;
    Comp comp[3];
    int16_t q[4][64];
    bool qset[4] = {false, false, false, false};
    // each component's table as it stood when the first scan that names the component started
    // (libjpeg's latch_quant_tables): a later DQT of the same id does not reach it
    int16_t qcomp[3][64];
    bool latched[3] = {false, false, false};
    Huff dc[4], ac[4];
    bool adobe = false;
    int adobe_transform = -1;
    bool jfif = false;

    // Parses and entropy-decodes into hd / binfo (per block: start, count) / coef (the caller's
    // scratch, reused across calls); returns the packet's byte size (write() lays it out).
    Header hd{};
    int64_t run(const uint8_t* d, size_t n, std::vector<uint32_t>& binfo, std::vector<uint32_t>& coef) {
        if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail("not a JPEG (no SOI)");
        size_t pos = 2;
        bool have_frame = false;
        hd = Header{};
        while (pos + 4 <= n) {
            if (d[pos] != 0xFF) {
                ++pos;
                continue;
            }
            const int m = d[pos + 1];
            if (m == 0xFF) {
                ++pos;
                continue;
            }
            pos += 2;
            if (m == 0xD9) break;                       // EOI
            if (m >= 0xD0 && m <= 0xD7) continue;       // stray RST
            if (pos + 2 > n) return fail("truncated marker");
            const int len = (d[pos] << 8) | d[pos + 1];
            if (len < 2 || pos + len > n) return fail("bad segment length");
            const uint8_t* s = d + pos + 2;
            const int sl = len - 2;
            if (m == 0xC0 || m == 0xC1) {  // baseline / extended sequential, Huffman
                if (sl < 6 || s[0] != 8) return unsupported("sample precision != 8");
                H = (s[1] << 8) | s[2];
                W = (s[3] << 8) | s[4];
                ncomp = s[5];
                if (H == 0 || W == 0) return unsupported("DNL height");
                if (ncomp != 1 && ncomp != 3) return unsupported("component count");
                if (sl < 6 + 3 * ncomp) return fail("short SOF");
                for (int c = 0; c < ncomp; ++c) {
                    comp[c].id = s[6 + 3 * c];
                    comp[c].h = s[7 + 3 * c] >> 4;
                    comp[c].v = s[7 + 3 * c] & 15;
                    comp[c].tq = s[8 + 3 * c] & 3;
                    if (comp[c].h < 1 || comp[c].v < 1 || comp[c].h > 4 || comp[c].v > 4) return fail("bad sampling");
                }
                hmax = vmax = 1;
                for (int c = 0; c < ncomp; ++c) {
                    hmax = std::max(hmax, comp[c].h);
                    vmax = std::max(vmax, comp[c].v);
                }
                if (ncomp == 3) {
                    // supported samplings: luma (hmax, vmax), chroma 1x1 with (hmax, vmax) in {1x1, 2x1, 2x2}
                    if (comp[0].h != hmax || comp[0].v != vmax || comp[1].h != 1 || comp[1].v != 1 ||
                        comp[2].h != 1 || comp[2].v != 1)
                        return unsupported("sampling factors");
                    if (!((hmax == 1 && vmax == 1) || (hmax == 2 && vmax == 1) || (hmax == 2 && vmax == 2)))
                        return unsupported("sampling factors");
                    // libjpeg's colour-space guess: RGB when Adobe transform 0, or no JFIF/Adobe and ids 'R','G','B'
                    if (adobe && adobe_transform == 0) return unsupported("RGB JPEG (Adobe transform 0)");
                    if (!jfif && !adobe && comp[0].id == 'R' && comp[1].id == 'G' && comp[2].id == 'B')
                        return unsupported("RGB JPEG");
                } else {
                    hmax = vmax = 1;  // a single component's sampling factors do not matter
                    comp[0].h = comp[0].v = 1;
                }
                hd.magic = PACKET_MAGIC;
                hd.version = PACKET_VERSION;
                hd.H = H;
                hd.W = W;
                hd.ncomp = ncomp;
                hd.hmax = hmax;
                hd.vmax = vmax;
                hd.mcus_x = (W + 8 * hmax - 1) / (8 * hmax);
                hd.mcus_y = (H + 8 * vmax - 1) / (8 * vmax);
                int nb = 0;
                for (int c = 0; c < ncomp; ++c) {
                    hd.h[c] = comp[c].h;
                    hd.v[c] = comp[c].v;
                    hd.bw[c] = hd.mcus_x * comp[c].h;
                    hd.bh[c] = hd.mcus_y * comp[c].v;
                    hd.cw[c] = (W * comp[c].h + hmax - 1) / hmax;  // downsampled_width (jdinput.c)
                    hd.ch[c] = (H * comp[c].v + vmax - 1) / vmax;
                    hd.block_base[c] = nb;
                    nb += hd.bw[c] * hd.bh[c];
                }
                hd.nblocks = nb;
                binfo.assign((size_t)2 * nb, 0u);
                coef.clear();
                coef.reserve((size_t)nb * 24);
                have_frame = true;
            } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
                return unsupported("progressive / lossless / arithmetic-coded JPEG");
            } else if (m == 0xC4) {  // DHT
                int p = 0;
                while (p < sl) {
                    if (p + 17 > sl) return fail("short DHT");
                    const int tc = s[p] >> 4, th = s[p] & 15;
                    uint8_t bits[17] = {0};
                    int cnt = 0;
                    for (int i = 1; i <= 16; ++i) {
                        bits[i] = s[p + i];
                        cnt += bits[i];
                    }
                    if (cnt > 256 || p + 17 + cnt > sl || th > 3 || tc > 1) return fail("bad DHT");
                    if (!build_huff(bits, s + p + 17, cnt, tc == 0 ? dc[th] : ac[th])) return fail("bad Huffman table");
                    p += 17 + cnt;
                }
            } else if (m == 0xDB) {  // DQT
                int p = 0;
                while (p < sl) {
                    const int pq = s[p] >> 4, tq = s[p] & 3;
                    if (pq == 0) {
                        if (p + 65 > sl) return fail("short DQT");
                        for (int k = 0; k < 64; ++k) q[tq][kNatural[k]] = s[p + 1 + k];
                        p += 65;
                    } else {
                        if (p + 129 > sl) return fail("short DQT");
                        for (int k = 0; k < 64; ++k) q[tq][kNatural[k]] = (int16_t)((s[p + 1 + 2 * k] << 8) | s[p + 2 + 2 * k]);
                        p += 129;
                    }
                    qset[tq] = true;
                }
            } else if (m == 0xDD) {  // DRI
                if (sl < 2) return fail("short DRI");
                restart = (s[0] << 8) | s[1];
            } else if (m == 0xE0) {
                if (sl >= 5 && std::memcmp(s, "JFIF\0", 5) == 0) jfif = true;
            } else if (m == 0xEE) {
                if (sl >= 12 && std::memcmp(s, "Adobe", 5) == 0) {
                    adobe = true;
                    adobe_transform = s[11];
                }
            } else if (m == 0xDA) {  // SOS
                if (!have_frame) return fail("SOS before SOF");
                const int ns = s[0];
                if (ns < 1 || ns > ncomp || sl < 1 + 2 * ns + 3) return fail("bad SOS");
                int sc[3], td[3], ta[3];
                for (int i = 0; i < ns; ++i) {
                    const int cid = s[1 + 2 * i];
                    sc[i] = -1;
                    for (int c = 0; c < ncomp; ++c)
                        if (comp[c].id == cid) sc[i] = c;
                    if (sc[i] < 0) return fail("SOS names an unknown component");
                    td[i] = s[2 + 2 * i] >> 4;
                    ta[i] = s[2 + 2 * i] & 15;
                    if (td[i] > 3 || ta[i] > 3 || !dc[td[i]].present || !ac[ta[i]].present) return fail("missing Huffman table");
                    // interleaved components follow the frame's order (T.81 B.2.3); libjpeg refuses others
                    if (i > 0 && sc[i] <= sc[i - 1]) return fail("SOS components out of frame order");
                }
                for (int i = 0; i < ns; ++i) {
                    const int c = sc[i];
                    if (latched[c]) continue;
                    if (!qset[comp[c].tq]) return fail("SOS names a component whose quantisation table is not defined yet");
                    std::memcpy(qcomp[c], q[comp[c].tq], sizeof(qcomp[c]));
                    latched[c] = true;
                }
                const int Ss = s[1 + 2 * ns], Se = s[2 + 2 * ns], AhAl = s[3 + 2 * ns];
                if (Ss != 0 || Se != 63 || AhAl != 0) return unsupported("spectral selection");
                pos += len;
                const int64_t used = scan(d + pos, n - pos, hd, ns, sc, td, ta, binfo, coef);
                if (used < 0) return -1;
                pos += (size_t)used;
                continue;
            }
            pos += len;
        }
        if (!have_frame) return fail("no frame");
        if (!latched[0] && !latched[1] && !latched[2]) return fail("no scan");
        // a component no scan named has no coefficients, and needs no table
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < 64; ++k) hd.quant[c][k] = c < ncomp && latched[c] ? qcomp[c][k] : 0;
        hd.nnz = (int32_t)coef.size();
        hd.off_blocks = (int32_t)((sizeof(Header) + 15) / 16 * 16);
        hd.off_coef = hd.off_blocks + 8 * hd.nblocks;
        const int64_t bytes = (int64_t)hd.off_coef + 4 * (int64_t)coef.size();
        if (bytes > 0x7fffffff) return fail("packet too large");
        hd.bytes = (int32_t)bytes;
        return bytes;
    }

    void write(uint8_t* out, const std::vector<uint32_t>& binfo, const std::vector<uint32_t>& coef) const {
        std::memset(out, 0, (size_t)hd.off_blocks);
        std::memcpy(out, &hd, sizeof(Header));
        std::memcpy(out + hd.off_blocks, binfo.data(), 4 * (size_t)2 * hd.nblocks);
        if (!coef.empty()) std::memcpy(out + hd.off_coef, coef.data(), 4 * coef.size());
    }

    // one scan; returns bytes consumed (up to the next marker that is not RST)
    int64_t scan(const uint8_t* d, size_t n, const Header& hd, int ns, const int* sc, const int* td, const int* ta,
                 std::vector<uint32_t>& binfo, std::vector<uint32_t>& coef) {
        BitReader br{d, n, 0};
        int pred[3] = {0, 0, 0};
        int mcus_x, mcus_y;
        if (ns == 1) {  // non-interleaved: one block per MCU over the component's own block grid
            const int c = sc[0];
            mcus_x = (hd.cw[c] + 7) / 8;
            mcus_y = (hd.ch[c] + 7) / 8;
        } else {
            mcus_x = hd.mcus_x;
            mcus_y = hd.mcus_y;
        }
        const int total = mcus_x * mcus_y;
        int todo = restart, next_rst = 0;
        for (int mcu = 0; mcu < total; ++mcu) {
            if (restart && todo == 0) {
                if (br.overran()) return fail("entropy data ends inside a restart interval");
                if (!br.restart_marker(next_rst)) return fail("restart marker missing or out of sequence");
                next_rst = (next_rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
                todo = restart;
            }
            const int my = mcu / mcus_x, mx = mcu % mcus_x;
            for (int i = 0; i < ns; ++i) {
                const int c = sc[i];
                const int bh = ns == 1 ? 1 : hd.v[c], bwn = ns == 1 ? 1 : hd.h[c];
                for (int by = 0; by < bh; ++by)
                    for (int bx = 0; bx < bwn; ++bx) {
                        const int row = ns == 1 ? my : my * hd.v[c] + by;
                        const int col = ns == 1 ? mx : mx * hd.h[c] + bx;
                        const int blk = hd.block_base[c] + row * hd.bw[c] + col;
                        if (decode_block(br, dc[td[i]], ac[ta[i]], pred[i], blk, binfo, coef)) return -1;
                    }
            }
            --todo;
        }
        if (br.overran()) return fail("entropy data ends inside the scan");
        // the scan ends at the next marker that is not a stuffed 0xFF00, a fill 0xFF or an RSTn: the
        // reader may stop short of it (bits already buffered), so search from where it stopped
        size_t p = std::min(br.pos, n);
        while (p + 1 < n) {
            if (d[p] == 0xFF && d[p + 1] != 0x00 && d[p + 1] != 0xFF && !(d[p + 1] >= 0xD0 && d[p + 1] <= 0xD7)) break;
            ++p;
        }
        return (int64_t)p;
    }

    int decode_block(BitReader& br, const Huff& dct, const Huff& act, int& pred, int blk, std::vector<uint32_t>& binfo,
                     std::vector<uint32_t>& coef) {
        const uint32_t start = (uint32_t)coef.size();
        const int s = decode_sym(br, dct);
        if (s < 0 || s > 11) {
            err = "bad DC code";
            return -1;
        }
        pred += extend(br.get(s), s);
        if (pred) coef.push_back(((uint32_t)(uint16_t)(int16_t)pred << 16) | 0u);
        for (int k = 1; k < 64;) {
            const int rs = decode_sym(br, act);
            if (rs < 0) {
                err = "bad AC code";
                return -1;
            }
            const int r = rs >> 4, sz = rs & 15;
            if (sz) {
                k += r;
                if (k > 63) {
                    err = "AC index past 63";
                    return -1;
                }
                const int v = extend(br.get(sz), sz);
                coef.push_back(((uint32_t)(uint16_t)(int16_t)v << 16) | (uint32_t)kNatural[k]);
                ++k;
            } else if (r == 15) {
                k += 16;
            } else {
                break;
            }
        }
        binfo[2 * (size_t)blk] = start;
        binfo[2 * (size_t)blk + 1] = (uint32_t)coef.size() - start;
        return 0;
    }

    int64_t fail(const char* m) {
        err = m;
        return -1;
    }
    int64_t unsupported(const char* m) {
        err = std::string("unsupported: ") + m;
        return 0;
    }
};

// ------------------------------------------------------------------------------------ reconstruction
// Device: blocks -> component planes.  Grid over (block groups of 8, image); the packet of image b
// starts at pk + off[b].  planes[b] holds the image's component planes (bw*8 x bh*8 bytes each, at
// plane offsets given by the header's block bases * 64).
__global__ void __launch_bounds__(256) jpeg_idct_kernel(const uint8_t* __restrict__ pk, const int64_t* __restrict__ off,
                                                        uint8_t* __restrict__ planes, int64_t plane_stride) {
    __shared__ int32_t tile[4][8][8 * 9];  // per wave: 8 blocks x (8 x 8 values, row pitch 9)
    const int b = blockIdx.y;
    const uint8_t* p = pk + off[b];
    const Header& hd = *reinterpret_cast<const Header*>(p);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int blk = (blockIdx.x * 4 + wave) * 8 + (lane >> 3);
    const int r = lane & 7;
    const bool valid = blk < hd.nblocks;  // (no early exit: every wave reaches the barriers)
    const uint32_t* binfo = reinterpret_cast<const uint32_t*>(p + hd.off_blocks);
    const uint32_t* coef = reinterpret_cast<const uint32_t*>(p + hd.off_coef);
    int c = 0;
    if (valid) c = blk >= hd.block_base[2] && hd.ncomp == 3 ? 2 : (blk >= hd.block_base[1] && hd.ncomp == 3 ? 1 : 0);
    int32_t* t = tile[wave][lane >> 3];
    // zero this block's 8 x 8 (lane r clears row r), then scatter its nonzero coefficients
#pragma unroll
    for (int j = 0; j < 8; ++j) t[r * 9 + j] = 0;
    __syncthreads();
    if (valid) {
        const uint32_t start = binfo[2 * blk], cnt = binfo[2 * blk + 1];
        for (uint32_t e = r; e < cnt; e += 8) {
            const uint32_t v = coef[start + e];
            const int idx = (int)(v & 63u);
            t[(idx >> 3) * 9 + (idx & 7)] = (int32_t)(int16_t)(v >> 16) * (int32_t)hd.quant[c][idx];
        }
    }
    __syncthreads();
    // pass 1: lane r = column r
    {
        int32_t col[8], w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) col[j] = t[j * 9 + r];
        idct_col(col, w);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j * 9 + r] = w[j];
    }
    __syncthreads();
    // pass 2: lane r = row r
    int32_t row[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) row[j] = t[r * 9 + j];
    uint8_t s[8];
    idct_row(row, s);
    if (!valid) return;
    const int local = blk - hd.block_base[c];
    const int by = local / hd.bw[c], bx = local - by * hd.bw[c];
    uint8_t* plane = planes + (int64_t)b * plane_stride + (int64_t)hd.block_base[c] * 64;
    uint64_t packed = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) packed |= (uint64_t)s[j] << (8 * j);
    *reinterpret_cast<uint64_t*>(plane + ((int64_t)(by * 8 + r) * hd.bw[c] + bx) * 8) = packed;
}

// one output pixel -> RGB, from the component planes of one image (host and device)
struct Planes {
    const uint8_t* base;
    const Header* hd;
};

EDGEDET_HD int sample(const Planes& P, int c, int y, int x) {
    const Header& hd = *P.hd;
    return P.base[(int64_t)hd.block_base[c] * 64 + (int64_t)y * hd.bw[c] * 8 + x];
}

// upsampled chroma sample of component c at output (y, x) (h2v2, h2v1 or none): fancy, except that a
// component of downsampled width 2 or less is replicated on both axes (jpeg_core.hpp; uniform per image)
EDGEDET_HD int chroma(const Planes& P, int c, int y, int x) {
    const Header& hd = *P.hd;
    const int cw = hd.cw[c], chh = hd.ch[c];
    if (hd.hmax == 1 && hd.vmax == 1) return sample(P, c, y, x);
    if (cw <= 2) return sample(P, c, hd.vmax == 1 ? y : y >> 1, x >> 1);
    if (hd.vmax == 1) {  // h2v1
        const int cx = x >> 1;
        const int in = sample(P, c, y, cx);
        if ((x & 1) == 0) return cx == 0 ? in : (in * 3 + sample(P, c, y, cx - 1) + 1) >> 2;
        return cx == cw - 1 ? in : (in * 3 + sample(P, c, y, cx + 1) + 2) >> 2;
    }
    // h2v2: nearest chroma row cy, next nearest above (even y) or below (odd y), edges replicated
    const int cy = y >> 1;
    int cy1 = (y & 1) ? cy + 1 : cy - 1;
    cy1 = cy1 < 0 ? 0 : (cy1 > chh - 1 ? chh - 1 : cy1);
    const int cx = x >> 1;
    auto colsum = [&](int cc) { return sample(P, c, cy, cc) * 3 + sample(P, c, cy1, cc); };
    const int t = colsum(cx);
    if ((x & 1) == 0) return cx == 0 ? (t * 4 + 8) >> 4 : (t * 3 + colsum(cx - 1) + 8) >> 4;
    return cx == cw - 1 ? (t * 4 + 7) >> 4 : (t * 3 + colsum(cx + 1) + 7) >> 4;
}

EDGEDET_HD void pixel(const Planes& P, int y, int x, uint8_t& r, uint8_t& g, uint8_t& b) {
    const int yy = sample(P, 0, y, x);
    if (P.hd->ncomp == 1) {
        r = g = b = (uint8_t)yy;
        return;
    }
    ycc_rgb(yy, chroma(P, 1, y, x), chroma(P, 2, y, x), r, g, b);
}

// device: planes -> out [B][3][H][W] uint8 (the batch all have the plan's H x W)
__global__ void __launch_bounds__(256) jpeg_color_kernel(const uint8_t* __restrict__ pk, const int64_t* __restrict__ off,
                                                         const uint8_t* __restrict__ planes, int64_t plane_stride,
                                                         uint8_t* __restrict__ out, int H, int W) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    Planes P{planes + (int64_t)b * plane_stride, reinterpret_cast<const Header*>(pk + off[b])};
    uint8_t r, g, bl;
    pixel(P, y, x, r, g, bl);
    uint8_t* o = out + (int64_t)b * 3 * H * W;
    o[i] = r;
    o[(int64_t)H * W + i] = g;
    o[2 * (int64_t)H * W + i] = bl;
}

// host reference of the same two stages (the checker entry)
static void reconstruct_host(const uint8_t* p, uint8_t* out) {
    const Header& hd = *reinterpret_cast<const Header*>(p);
    std::vector<uint8_t> planes((size_t)hd.nblocks * 64);
    const uint32_t* binfo = reinterpret_cast<const uint32_t*>(p + hd.off_blocks);
    const uint32_t* coef = reinterpret_cast<const uint32_t*>(p + hd.off_coef);
    for (int blk = 0; blk < hd.nblocks; ++blk) {
        const int c = hd.ncomp == 3 && blk >= hd.block_base[2] ? 2 : (hd.ncomp == 3 && blk >= hd.block_base[1] ? 1 : 0);
        int32_t t[64] = {0};
        for (uint32_t e = 0; e < binfo[2 * blk + 1]; ++e) {
            const uint32_t v = coef[binfo[2 * blk] + e];
            const int idx = (int)(v & 63u);
            t[idx] = (int32_t)(int16_t)(v >> 16) * (int32_t)hd.quant[c][idx];
        }
        int32_t w[64];
        for (int col = 0; col < 8; ++col) {
            int32_t cv[8], o[8];
            for (int j = 0; j < 8; ++j) cv[j] = t[j * 8 + col];
            idct_col(cv, o);
            for (int j = 0; j < 8; ++j) w[j * 8 + col] = o[j];
        }
        const int local = blk - hd.block_base[c];
        const int by = local / hd.bw[c], bx = local - by * hd.bw[c];
        for (int r = 0; r < 8; ++r) {
            uint8_t s[8];
            idct_row(w + r * 8, s);
            std::memcpy(&planes[(size_t)hd.block_base[c] * 64 + ((size_t)(by * 8 + r) * hd.bw[c] + bx) * 8], s, 8);
        }
    }
    Planes P{planes.data(), &hd};
    const int64_t HW = (int64_t)hd.H * hd.W;
    for (int y = 0; y < hd.H; ++y)
        for (int x = 0; x < hd.W; ++x) {
            uint8_t r, g, b;
            pixel(P, y, x, r, g, b);
            const int64_t i = (int64_t)y * hd.W + x;
            out[i] = r;
            out[HW + i] = g;
            out[2 * HW + i] = b;
        }
}

}  // namespace jpeg
}  // namespace edgedet

using namespace edgedet;
using namespace edgedet::jpeg;

// Entropy-decode one JPEG file image (bytes) into a packet.  Returns the packet size (and writes it
// when cap is large enough), 0 = a JPEG this decoder does not handle (the caller decodes it on the
// host; edgedet_last_error says why), < 0 = malformed data.  Thread-safe; host only.
extern "C" int64_t edgedet_jpeg_packet(const uint8_t* data, int64_t size, void* out, int64_t cap, int32_t* hw) {
    EDGEDET_REQUIRE(data && size > 0, "jpeg_packet: empty input");
    // per-thread scratch, kept across calls (a host thread decodes file after file)
    static thread_local std::vector<uint32_t> binfo, coef;
    Decoder dec;
    const int64_t n = dec.run(data, (size_t)size, binfo, coef);
    if (n <= 0) {
        set_error("edgedet: jpeg: " + dec.err);
        return n;
    }
    if (hw) {
        hw[0] = dec.H;
        hw[1] = dec.W;
    }
    if (out && cap >= n) dec.write(static_cast<uint8_t*>(out), binfo, coef);
    return n;
}

// One batch of JPEG files -> the device image edgedet_jpeg_decode_batch reads, on `threads` host threads
// (0 = hardware concurrency), in one call: out[0 .. 8n) = the packet offsets (int64, from out), padded to
// 256 B, then the packets, each 256-B aligned (placed in completion order; the offsets say where).
// hw[2i..2i+1] = (H, W) of file i; *max_plane_bytes = the largest nblocks * 64 of the batch.  Returns the
// bytes the batch image spans (the upload); when that exceeds `cap` nothing usable was written and the
// caller retries with a buffer of the returned size.  0 = a file the device path does not handle or
// rejects as malformed (the caller decodes the batch on the host; edgedet_last_error says which and
// why), < 0 = a file that cannot be opened or read.  Replaces a Python thread pool calling edgedet_jpeg_packet per file, whose per-file
// Python work and pinned allocations kept the detect CLI at a quarter of the entropy decoders' rate.
extern "C" int64_t edgedet_jpeg_batch_packets(const char* const* paths, int64_t n, void* out, int64_t cap,
                                              int32_t* hw, int64_t* max_plane_bytes, int32_t threads) {
    EDGEDET_REQUIRE(n >= 1 && paths && hw && max_plane_bytes && (out || cap == 0), "jpeg_batch_packets: bad arguments");
    const int64_t head = (8 * n + 255) / 256 * 256;
    int nt = threads > 0 ? threads : (int)std::max(1u, std::thread::hardware_concurrency());
    nt = (int)std::min<int64_t>(nt, n);
    std::atomic<int64_t> next{0}, used{head}, planes{0};
    std::atomic<int> status{1};  // 1 ok, 0 unsupported, < 0 error (first one wins)
    std::string why;
    std::atomic<bool> why_set{false};
    auto fail = [&](int st, const std::string& msg) {
        int expect = 1;
        if (status.compare_exchange_strong(expect, st) && !why_set.exchange(true)) why = msg;
    };
    int64_t* offs = static_cast<int64_t*>(out);
    auto work = [&] {
        static thread_local std::vector<uint32_t> binfo, coef;
        static thread_local std::vector<uint8_t> file;
        int64_t i;
        while ((i = next.fetch_add(1)) < n && status.load(std::memory_order_relaxed) == 1) {
            FILE* f = paths[i] ? std::fopen(paths[i], "rb") : nullptr;
            if (!f) {
                fail(-1, std::string("edgedet: jpeg: cannot open ") + (paths[i] ? paths[i] : "(null)"));
                return;
            }
            std::fseek(f, 0, SEEK_END);
            const long sz = std::ftell(f);
            std::fseek(f, 0, SEEK_SET);
            file.resize(sz > 0 ? (size_t)sz : 1);
            const size_t got = sz > 0 ? std::fread(file.data(), 1, (size_t)sz, f) : 0;
            std::fclose(f);
            if (sz <= 0 || got != (size_t)sz) {
                fail(-1, std::string("edgedet: jpeg: cannot read ") + paths[i]);
                return;
            }
            Decoder dec;
            const int64_t m = dec.run(file.data(), file.size(), binfo, coef);
            if (m <= 0) {
                // a file this decoder rejects — unsupported, not a JPEG at all (a PNG named .jpg), or
                // entropy data it cannot parse (libjpeg only warns on those and still decodes) — makes
                // the batch "unsupported": the caller decodes it on the host, as the reference's
                // read_image would.  Only an unreadable file is an error.
                fail(0, std::string("edgedet: jpeg: ") + paths[i] + ": " + (m == 0 ? "" : "rejected: ") + dec.err);
                return;
            }
            hw[2 * i] = dec.H;
            hw[2 * i + 1] = dec.W;
            int64_t pb = (int64_t)dec.hd.nblocks * 64, cur = planes.load();
            while (pb > cur && !planes.compare_exchange_weak(cur, pb)) {
            }
            const int64_t off = used.fetch_add((m + 255) / 256 * 256);
            if (off + m <= cap) {
                dec.write(static_cast<uint8_t*>(out) + off, binfo, coef);
                offs[i] = off;
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    if (status.load() != 1) {
        set_error(why);
        return status.load();
    }
    *max_plane_bytes = planes.load();
    return used.load();
}

// (H, W) of an image file from its header, as PIL's Image.open(path).size reports it (detect.py's
// read_image shapes; EXIF orientation is not applied by either): JPEG from the first SOFn segment, PNG
// from IHDR.  1 = found, 0 = another format or no SOF in the first 1 MiB (the caller asks PIL).
static int image_dims(const char* path, int32_t* hw) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 0;
    uint8_t buf[65536];
    size_t want = 4096;  // the frame header is usually in the first few hundred bytes
    size_t n = std::fread(buf, 1, want, f);
    bool eof = n < want;
    int found = 0;
    if (n >= 24 && std::memcmp(buf, "\x89PNG\r\n\x1a\n", 8) == 0 && std::memcmp(buf + 12, "IHDR", 4) == 0) {
        hw[1] = (int32_t)(((uint32_t)buf[16] << 24) | ((uint32_t)buf[17] << 16) | ((uint32_t)buf[18] << 8) | buf[19]);
        hw[0] = (int32_t)(((uint32_t)buf[20] << 24) | ((uint32_t)buf[21] << 16) | ((uint32_t)buf[22] << 8) | buf[23]);
        found = 1;
    } else if (n >= 4 && buf[0] == 0xFF && buf[1] == 0xD8) {
        // walk the marker segments; a segment may straddle the buffer end: refill from its start
        size_t base = 0, pos = 2;  // file offset of buf[0]; position in buf
        for (int guard = 0; guard < 4096 && !found; ++guard) {
            if (pos + 9 > n) {
                if (eof || base + pos > (1u << 20)) break;
                base += pos;
                if (std::fseek(f, (long)base, SEEK_SET) != 0) break;
                want = sizeof(buf);
                n = std::fread(buf, 1, want, f);
                eof = n < want;
                pos = 0;
                if (n < 9) break;
            }
            if (buf[pos] != 0xFF) break;
            const int m = buf[pos + 1];
            if (m == 0xFF) {  // fill byte
                ++pos;
                continue;
            }
            if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) {  // no length
                pos += 2;
                continue;
            }
            const size_t len = ((size_t)buf[pos + 2] << 8) | buf[pos + 3];
            if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
                hw[0] = (int32_t)(((uint32_t)buf[pos + 5] << 8) | buf[pos + 6]);
                hw[1] = (int32_t)(((uint32_t)buf[pos + 7] << 8) | buf[pos + 8]);
                found = hw[0] > 0 && hw[1] > 0;
                break;
            }
            if (m == 0xD9 || m == 0xDA || len < 2) break;  // EOI / scan before any frame header
            pos += 2 + len;
        }
    }
    std::fclose(f);
    return found;
}

// Header dims of n files on `threads` host threads (0 = hardware concurrency): hw[2i..2i+1] = (H, W),
// or (0, 0) where the header was not understood.  Returns how many were found.
extern "C" int64_t edgedet_image_dims(const char* const* paths, int64_t n, int32_t* hw, int32_t threads) {
    EDGEDET_REQUIRE(n >= 0 && (n == 0 || (paths && hw)), "image_dims: null arguments");
    int nt = threads > 0 ? threads : (int)std::max(1u, std::thread::hardware_concurrency());
    nt = (int)std::min<int64_t>(nt, std::max<int64_t>(1, n / 16));
    std::atomic<int64_t> next{0}, found{0};
    auto work = [&] {
        int64_t k;
        while ((k = next.fetch_add(64)) < n)
            for (int64_t i = k; i < std::min<int64_t>(n, k + 64); ++i) {
                hw[2 * i] = hw[2 * i + 1] = 0;
                if (paths[i] && image_dims(paths[i], hw + 2 * i)) found.fetch_add(1);
            }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return found.load();
}

// Plane scratch bytes one image of the batch needs: the largest nblocks * 64 over the packets is what
// edgedet_jpeg_decode_batch's plane_stride must cover (host helper, reads a host packet).
extern "C" int64_t edgedet_jpeg_plane_bytes(const void* host_packet) {
    EDGEDET_REQUIRE(host_packet, "jpeg_plane_bytes: null packet");
    const Header& hd = *reinterpret_cast<const Header*>(host_packet);
    EDGEDET_REQUIRE(hd.magic == PACKET_MAGIC && hd.version == PACKET_VERSION, "jpeg_plane_bytes: not a packet");
    return (int64_t)hd.nblocks * 64;
}

// Device decode of B packets (device copies at packets + offsets[b]; the headers of the host copies are
// checked by the caller) into out [B][3][H][W] uint8 — torchvision read_image(..., RGB) layout, the
// detector plan's uint8 input.  planes: scratch of B * plane_stride bytes.  max_blocks: the largest
// block count of the batch (grid size).  Asynchronous on `stream`.
extern "C" int edgedet_jpeg_decode_batch(const void* packets, const int64_t* offsets, int32_t B, int32_t H, int32_t W,
                                         int32_t max_blocks, void* planes, int64_t plane_stride, uint8_t* out,
                                         void* stream) {
    EDGEDET_REQUIRE(packets && offsets && planes && out && B >= 1 && H >= 1 && W >= 1 && max_blocks >= 1,
                    "jpeg_decode_batch: bad arguments");
    EDGEDET_REQUIRE(plane_stride >= (int64_t)max_blocks * 64 && plane_stride % 8 == 0,
                    "jpeg_decode_batch: plane stride below 64 bytes per block (or not 8-byte aligned)");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)cdiv(max_blocks, 32), (unsigned)B), dim3(256), 0, s,
                       (const uint8_t*)packets, offsets, (uint8_t*)planes, plane_stride);
    EDGEDET_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)cdiv((int64_t)H * W, 256), (unsigned)B), dim3(256), 0, s,
                       (const uint8_t*)packets, offsets, (const uint8_t*)planes, plane_stride, out, H, W);
    EDGEDET_LAUNCH_CHECK();
    return 0;
}

// The same reconstruction on the host, from a host packet, into out [3][H][W]: the checker the CPU
// tests pin against the reference decoder (not on any product path).
extern "C" int edgedet_jpeg_reconstruct_host(const void* host_packet, uint8_t* out) {
    EDGEDET_REQUIRE(host_packet && out, "jpeg_reconstruct_host: null pointer");
    const Header& hd = *reinterpret_cast<const Header*>(host_packet);
    EDGEDET_REQUIRE(hd.magic == PACKET_MAGIC && hd.version == PACKET_VERSION, "jpeg_reconstruct_host: not a packet");
    reconstruct_host((const uint8_t*)host_packet, out);
    return 0;
}
