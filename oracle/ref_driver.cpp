// TEST INFRASTRUCTURE ONLY.  Drives the reference's own ErasureCode classes (its rs.h / lrc.h / pc.h, included at
// compile time only; none of its text is here) over a request file and writes what they returned.
//
//   ref_driver REQUEST INPUT RESULT
//
// REQUEST is text, one operation per line (tests/reference_ec_cases.py writes it); INPUT is the bytes the data blocks
// are cut from (block i of size B is INPUT[i * 1029, i * 1029 + B)); RESULT gets one JSON line per request line, in
// order, flushed after each, so a process the reference ends (utils.cpp's my_assert exits) leaves every earlier answer.
//
//   code T k m l g k1 m1 k2 m2 x seri_num isvertical   construct class T (the ECTYPE number), init_coding_parameters,
//                                                      get_coding_parameters, k, m
//   mat                                                make_encoding_matrix into m * k ints preset to -1
//   part F|O                                           placement_rule, generate_partition, partition_plan
//   enc B                                              encode; the stripe of size B stays for the lines below
//   add B block_num parity_num                         perform_addition over the stripe's first block_num blocks
//   pat F|O SIZES n f1..fn                             check_if_decodable, generate_repair_plan and, where decodable,
//                                                      decode at each size of SIZES (bit 0: 80, bit 1: 1029)
//   pdec B loc nl l.. ns s.. nf f..                    encode_partial_blocks_for_decoding, local_or_column = loc
//   penc B loc nd d.. np p..                           encode_partial_blocks_for_encoding, local_or_column = loc
//
// Built twice by oracle/Makefile: against ref_cpu_backend.c (CPU) and against libecg.so (INTEGRATION.md Option A).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "rs.h"
#include "lrc.h"
#include "pc.h"

using namespace ECProject;

namespace {

constexpr int kSlot = 1029;  // stride of the data blocks inside INPUT
constexpr unsigned char kErased = 0xE7;

// ---- SHA-256 (FIPS 180-4)
struct Sha256 {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    unsigned char buf[64];
    size_t fill = 0;
    uint64_t total = 0;

    static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

    void block(const unsigned char* p) {
        static const uint32_t K[64] = {
            0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
            0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
            0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
            0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
            0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
            0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
            0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
            0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
        uint32_t w[64];
        for (int i = 0; i < 16; i++)
            w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
        for (int i = 16; i < 64; i++) {
            const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
            const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
            w[i] = w[i - 16] + s0 + w[i - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; i++) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }

    void update(const void* data, size_t n) {
        const unsigned char* p = (const unsigned char*)data;
        total += n;
        while (n > 0) {
            const size_t take = std::min(n, sizeof(buf) - fill);
            memcpy(buf + fill, p, take);
            fill += take; p += take; n -= take;
            if (fill == 64) { block(buf); fill = 0; }
        }
    }

    std::string hex() {
        const uint64_t bits = total * 8;
        const unsigned char one = 0x80, zero = 0;
        update(&one, 1);
        while (fill != 56) update(&zero, 1);
        unsigned char len[8];
        for (int i = 0; i < 8; i++) len[i] = (unsigned char)(bits >> (56 - 8 * i));
        update(len, 8);
        char out[65];
        for (int i = 0; i < 8; i++) snprintf(out + 8 * i, 9, "%08x", h[i]);
        return std::string(out, 64);
    }
};

using Block = std::vector<char>;

std::string block_json(const Block& b) {  // ["<sha-256>", "<first 16 bytes>"]
    Sha256 s;
    s.update(b.data(), b.size());
    std::string head;
    char t[3];
    for (size_t i = 0; i < b.size() && i < 16; i++) {
        snprintf(t, sizeof t, "%02x", (unsigned char)b[i]);
        head += t;
    }
    return "[\"" + s.hex() + "\",\"" + head + "\"]";
}

std::string blocks_json(const std::vector<Block>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + block_json(v[i]);
    return s + "]";
}

std::string ints_json(const std::vector<int>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
    return s + "]";
}

std::string lists_json(const std::vector<std::vector<int>>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + ints_json(v[i]);
    return s + "]";
}

std::vector<int> read_ints(std::istringstream& in) {
    int n = 0;
    in >> n;
    std::vector<int> v(n);
    for (auto& x : v) in >> x;
    return v;
}

struct State {
    std::unique_ptr<ErasureCode> ec;
    std::vector<char> input;
    std::map<int, std::vector<Block>> stripes;  // block size -> the k + m blocks as encode left them
};

// The classes by ECTYPE, constructed as the reference's own factory constructs them (ERS and HPC take the rest of
// their parameters from init_coding_parameters).
ErasureCode* make_code(int type, const CodingParameters& cp, bool isvertical) {
    switch (type) {
        case RS: return new RSCode(cp.k, cp.m);
        case ERS: return new EnlargedRSCode(cp.k, cp.m);
        case AZURE_LRC: return new Azu_LRC(cp.k, cp.l, cp.g);
        case AZURE_LRC_1: return new Azu_LRC_1(cp.k, cp.l, cp.g);
        case OPTIMAL_LRC: return new Opt_LRC(cp.k, cp.l, cp.g);
        case OPTIMAL_CAUCHY_LRC: {
            // The class never initialises surviving_group_id, and its plan for one lost global parity reads it
            // before anything sets it: what the plan says then depends on what the heap held.  Group 0 is what a
            // fresh process gives and what the project assumes; without this line the record would not reproduce.
            Opt_Cau_LRC* c = new Opt_Cau_LRC(cp.k, cp.l, cp.g);
            c->surviving_group_id = 0;
            return c;
        }
        case UNIFORM_CAUCHY_LRC: return new Uni_Cau_LRC(cp.k, cp.l, cp.g);
        case PC: return new ProductCode(cp.k1, cp.m1, cp.k2, cp.m2);
        case Hierachical_PC: {
            HPC* h = new HPC(cp.k1, cp.m1, cp.k2, cp.m2);
            h->isvertical = isvertical;
            return h;
        }
        case HV_PC: return new HVPC(cp.k1, cp.m1, cp.k2, cp.m2);
    }
    return nullptr;
}

void split(std::vector<Block>& blocks, int k, std::vector<char*>& data, std::vector<char*>& coding) {
    for (size_t i = 0; i < blocks.size(); i++) ((int)i < k ? data : coding).push_back(blocks[i].data());
}

std::string op_code(State& st, std::istringstream& in) {
    int type = 0, isv = 1;
    CodingParameters cp;
    in >> type >> cp.k >> cp.m >> cp.l >> cp.g >> cp.k1 >> cp.m1 >> cp.k2 >> cp.m2 >> cp.x >> cp.seri_num >> isv;
    st.stripes.clear();
    st.ec.reset(make_code(type, cp, isv != 0));
    if (!st.ec) return "{\"error\":\"no such ECTYPE\"}";
    st.ec->init_coding_parameters(cp);
    CodingParameters got;
    got.k = got.m = got.l = got.g = got.k1 = got.m1 = got.k2 = got.m2 = got.x = got.seri_num = -1;
    st.ec->get_coding_parameters(got);
    const std::vector<int> f = {got.k, got.m, got.l, got.g, got.k1, got.m1, got.k2, got.m2, got.x, got.seri_num,
                                got.local_or_column ? 1 : 0};
    return "{\"k\":" + std::to_string(st.ec->k) + ",\"m\":" + std::to_string(st.ec->m) + ",\"cp\":" + ints_json(f) + "}";
}

std::string op_mat(State& st) {
    std::vector<int> m((size_t)st.ec->k * st.ec->m, -1);
    st.ec->make_encoding_matrix(m.data());
    return "{\"matrix\":" + ints_json(m) + "}";
}

void place(State& st, const std::string& rule) {
    const PlacementRule want = rule == "F" ? FLAT : OPTIMAL;
    if (st.ec->placement_rule != want || st.ec->partition_plan.empty()) {
        st.ec->placement_rule = want;
        st.ec->generate_partition();
    }
}

std::string op_part(State& st, std::istringstream& in) {
    std::string rule;
    in >> rule;
    st.ec->placement_rule = rule == "F" ? FLAT : OPTIMAL;
    st.ec->generate_partition();
    return "{\"partition\":" + lists_json(st.ec->partition_plan) + "}";
}

std::string op_enc(State& st, std::istringstream& in) {
    int B = 0;
    in >> B;
    const int k = st.ec->k, m = st.ec->m;
    std::vector<Block> blocks(k + m, Block(B, 0));
    for (int i = 0; i < k; i++) memcpy(blocks[i].data(), st.input.data() + (size_t)i * kSlot, B);
    std::vector<char*> data, coding;
    split(blocks, k, data, coding);
    st.ec->encode(data.data(), coding.data(), B);
    std::vector<Block> parities(blocks.begin() + k, blocks.end());
    st.stripes[B] = blocks;
    return "{\"out\":" + blocks_json(parities) + "}";
}

std::string op_add(State& st, std::istringstream& in) {
    int B = 0, block_num = 0, parity_num = 0;
    in >> B >> block_num >> parity_num;
    std::vector<Block>& stripe = st.stripes.at(B);
    std::vector<Block> out(parity_num, Block(B, 0));
    std::vector<char*> data, coding;
    for (int i = 0; i < block_num; i++) data.push_back(stripe[i].data());
    for (auto& b : out) coding.push_back(b.data());
    st.ec->perform_addition(data.data(), coding.data(), B, block_num, parity_num);
    return "{\"out\":" + blocks_json(out) + "}";
}

std::string op_pat(State& st, std::istringstream& in) {
    std::string rule;
    int sizes = 0;
    in >> rule >> sizes;
    const std::vector<int> fails = read_ints(in);
    place(st, rule);
    const bool decodable = st.ec->check_if_decodable(fails);
    std::vector<RepairPlan> plans;
    const bool ret = st.ec->generate_repair_plan(fails, plans);
    st.ec->local_or_column = false;  // the LRC planner leaves its last plan's flag behind
    std::string s = std::string("{\"dec\":") + (decodable ? "1" : "0") + ",\"ret\":" + (ret ? "1" : "0") + ",\"plans\":[";
    for (size_t i = 0; i < plans.size(); i++)
        s += std::string(i ? "," : "") + "[" + (plans[i].local_or_column ? "1" : "0") + "," +
             ints_json(plans[i].failure_idxs) + "," + lists_json(plans[i].help_blocks) + "]";
    s += "],\"d\":{";
    bool first = true;
    const int both[2] = {80, 1029};
    for (int b = 0; b < 2 && decodable; b++) {
        if (!(sizes >> b & 1)) continue;
        const int B = both[b], k = st.ec->k, n = st.ec->k + st.ec->m;
        std::vector<Block> blocks = st.stripes.at(B);
        for (int f : fails) memset(blocks[f].data(), kErased, B);
        std::vector<int> erasures(fails);
        erasures.resize(n + 1, -1);
        std::vector<char*> data, coding;
        split(blocks, k, data, coding);
        st.ec->decode(data.data(), coding.data(), B, erasures.data(), (int)fails.size());
        std::vector<Block> lost;
        Sha256 all;
        for (int f : fails) lost.push_back(blocks[f]);
        for (auto& blk : blocks) all.update(blk.data(), blk.size());
        s += std::string(first ? "" : ",") + "\"" + std::to_string(B) + "\":{\"out\":" + blocks_json(lost) +
             ",\"all\":\"" + all.hex() + "\"}";
        first = false;
    }
    return s + "}}";
}

std::string op_partial(State& st, std::istringstream& in, bool decoding) {
    int B = 0, loc = 0;
    in >> B >> loc;
    const std::vector<int> a = read_ints(in), b = read_ints(in);
    const std::vector<int> c = decoding ? read_ints(in) : std::vector<int>();
    std::vector<Block>& stripe = st.stripes.at(B);
    std::vector<Block> out(decoding ? c.size() : b.size(), Block(B, 0));
    std::vector<char*> data, coding;
    for (int i : a) data.push_back(stripe[i].data());
    for (auto& blk : out) coding.push_back(blk.data());
    st.ec->local_or_column = loc != 0;
    if (decoding)
        st.ec->encode_partial_blocks_for_decoding(data.data(), coding.data(), B, a, b, c);
    else
        st.ec->encode_partial_blocks_for_encoding(data.data(), coding.data(), B, a, b);
    st.ec->local_or_column = false;
    return "{\"out\":" + blocks_json(out) + "}";
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s REQUEST INPUT RESULT\n", argv[0]);
        return 2;
    }
    std::ifstream req(argv[1]);
    std::ifstream inp(argv[2], std::ios::binary);
    FILE* res = fopen(argv[3], "w");
    if (!req || !inp || !res) {
        fprintf(stderr, "cannot open the request, input or result file\n");
        return 2;
    }
    State st;
    st.input.assign(std::istreambuf_iterator<char>(inp), std::istreambuf_iterator<char>());
    std::string line;
    while (std::getline(req, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string op, out;
        in >> op;
        if (op == "code") out = op_code(st, in);
        else if (!st.ec) out = "{\"error\":\"no code\"}";
        else if (op == "mat") out = op_mat(st);
        else if (op == "part") out = op_part(st, in);
        else if (op == "enc") out = op_enc(st, in);
        else if (op == "add") out = op_add(st, in);
        else if (op == "pat") out = op_pat(st, in);
        else if (op == "pdec") out = op_partial(st, in, true);
        else if (op == "penc") out = op_partial(st, in, false);
        else out = "{\"error\":\"unknown operation\"}";
        fputs(out.c_str(), res);
        fputc('\n', res);
        fflush(res);
    }
    fclose(res);
    return 0;
}
