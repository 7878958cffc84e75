// expr_host_main.cpp — the host build of databend_amd/csrc/expr.hpp as a program of its own, for a
// run under -fsanitize=address,undefined (tests/test_expr_host.py).  Nothing here is loaded into Python.
//
//   expr_host_main <cases.bin> <out.txt>
//   expr_host_main --programs <programs.bin> <out.txt>      (whole programs, described at run_programs)
//
// cases.bin: u32 count, then per case
//   u8 op (0 plus, 1 minus, 2 multiply), u8 type_a, u8 precision_a, u8 scale_a, u8 type_b, u8 precision_b, u8 scale_b, u8 pad,
//   u64 a_lo, a_hi, b_lo, b_hi      canonical operands: integers extended to 128 bits, floats as the bits of a double
// Each case is compiled as the program [COLUMN 0, COLUMN 1, op, STORE 0] through expr_compile and its
// operator node is run on the operands.  out.txt, one line per case:
//   "<status> <type> <precision> <scale> <lo hex> <hi hex> <error 0/1>"   (status != 0: the rest is zeros)
// Every case's nodes and columns live in heap blocks of exactly their size.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "expr.hpp"

static bool read_all(const char* path, std::vector<uint8_t>& buf) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    buf.resize((size_t)n);
    const bool ok = n == 0 || fread(buf.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

// --programs: whole multi-node programs, one output each, run row by row over a plain vector stack
// with the same per-row operators (expr_num + expr_num_hi, expr_dec_add, expr_dec_mul).
//   u32 count; per program: u16 n_cols, u16 n_nodes, u32 n_rows;
//   n_cols x (u8 type, precision, scale, nullable);
//   n_nodes x (u8 kind (0 column, 1 constant, 2 plus, 3 minus, 4 multiply), u8 column, u8 type, precision, scale, 3 pad, u64 lo, hi);
//   n_rows x n_cols x (u64 valid, lo, hi)   canonical cells
// The output is stored after the last node.  One line per row: "<status> <type> <precision> <scale> <lo hex> <hi hex> <valid> <error>".
struct HostVal {
    uint64_t lo, hi;
    bool valid;
};

static int run_programs(const std::vector<uint8_t>& in, FILE* out) {
    size_t at = 4;
    uint32_t count;
    memcpy(&count, in.data(), 4);
    for (uint32_t i = 0; i < count; ++i) {
        uint16_t n_cols, n_nodes;
        uint32_t n_rows;
        if (at + 8 > in.size()) return 2;
        memcpy(&n_cols, &in[at], 2), memcpy(&n_nodes, &in[at + 2], 2), memcpy(&n_rows, &in[at + 4], 4);
        at += 8;
        const size_t need = (size_t)n_cols * 4 + (size_t)n_nodes * 24 + (size_t)n_rows * n_cols * 24;
        if (at + need > in.size()) return 2;
        std::unique_ptr<dbg_column[]> cols(new dbg_column[n_cols]);
        memset(cols.get(), 0, n_cols * sizeof(dbg_column));
        for (int c = 0; c < n_cols; ++c, at += 4)
            cols[c].dt.type = in[at], cols[c].dt.precision = in[at + 1], cols[c].dt.scale = in[at + 2], cols[c].dt.nullable = in[at + 3];
        std::unique_ptr<dbg_expr_node[]> nodes(new dbg_expr_node[n_nodes + 1]);
        memset(nodes.get(), 0, (n_nodes + 1) * sizeof(dbg_expr_node));
        static const int kinds[5] = {DBG_EXPR_COLUMN, DBG_EXPR_CONST, DBG_EXPR_PLUS, DBG_EXPR_MINUS, DBG_EXPR_MULTIPLY};
        for (int k = 0; k < n_nodes; ++k, at += 24) {
            dbg_expr_node& n = nodes[k];
            n.op = in[at] < 5 ? kinds[in[at]] : 99;
            n.index = in[at + 1];
            n.dt.type = in[at + 2], n.dt.precision = in[at + 3], n.dt.scale = in[at + 4];
            uint64_t lo, hi;
            memcpy(&lo, &in[at + 8], 8), memcpy(&hi, &in[at + 16], 8);
            n.i64 = (int64_t)lo, n.i128_lo = lo, n.i128_hi = (int64_t)hi;
            n.f64 = expr_bits_f64(lo);
        }
        nodes[n_nodes].op = DBG_EXPR_STORE, nodes[n_nodes].index = 0;
        dbg_expr_program prog;
        memset(&prog, 0, sizeof(prog));
        prog.nodes = nodes.get(), prog.n_nodes = n_nodes + 1, prog.cols = cols.get(), prog.n_cols = n_cols, prog.n_outputs = 1;
        ExprCompiled C;
        std::string msg;
        const int rc = expr_compile(&prog, C, msg);
        const dbg_datatype t = C.out_types[0];
        for (uint32_t r = 0; r < n_rows; ++r, at += (size_t)n_cols * 24) {
            if (rc != DBG_OK) {
                fprintf(out, "%d 0 0 0 0 0 0 0\n", rc);
                continue;
            }
            std::vector<HostVal> st;
            HostVal stored{0, 0, false};
            bool err = false;
            for (const ENode& n : C.nodes) {
                if (n.op == EX_COL) {
                    uint64_t cell[3];
                    memcpy(cell, &in[at + (size_t)n.idx * 24], 24);
                    st.push_back(HostVal{cell[1], cell[2], cell[0] != 0});
                } else if (n.op == EX_CONST) {
                    st.push_back(HostVal{n.c[0], n.c[1], true});
                } else if (n.op == EX_STORE) {
                    stored = st.back();
                    if (n.flags & EX_F_POP) st.pop_back();
                } else {
                    const HostVal b = st.back();
                    st.pop_back();
                    const HostVal a = st.back();
                    st.pop_back();
                    HostVal v{0, 0, a.valid && b.valid};
                    bool bad = false;
                    if (n.op == EX_NUM) {
                        v.lo = expr_num(n, a.lo, b.lo);
                        v.hi = expr_num_hi(n, v.lo);
                    } else {
                        const EU128 q = n.op == EX_DADD ? expr_dec_add(n, EU128{a.lo, a.hi}, EU128{b.lo, b.hi}, &bad)
                                                        : expr_dec_mul(n, EU128{a.lo, a.hi}, EU128{b.lo, b.hi}, &bad);
                        v.lo = q.lo, v.hi = q.hi;
                    }
                    if (bad && v.valid) err = true;
                    st.push_back(v);
                }
            }
            fprintf(out, "0 %d %d %d %llx %llx %d %d\n", t.type, t.precision, t.scale, (unsigned long long)stored.lo,
                    (unsigned long long)stored.hi, stored.valid ? 1 : 0, err ? 1 : 0);
        }
    }
    return at == in.size() ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc == 4 && strcmp(argv[1], "--programs") == 0) {
        std::vector<uint8_t> in;
        if (!read_all(argv[2], in) || in.size() < 4) return 2;
        FILE* out = fopen(argv[3], "w");
        if (!out) return 2;
        const int rc = run_programs(in, out);
        fclose(out);
        return rc;
    }
    if (argc != 3) {
        fprintf(stderr, "usage: expr_host_main <cases.bin> <out.txt>\n");
        return 2;
    }
    std::vector<uint8_t> in;
    if (!read_all(argv[1], in) || in.size() < 4) return 2;
    uint32_t count;
    memcpy(&count, in.data(), 4);
    const size_t rec = 8 + 32;
    if (in.size() != 4 + (size_t)count * rec) {
        fprintf(stderr, "bad case file\n");
        return 2;
    }
    FILE* out = fopen(argv[2], "w");
    if (!out) return 2;
    static const int ops[3] = {DBG_EXPR_PLUS, DBG_EXPR_MINUS, DBG_EXPR_MULTIPLY};
    for (uint32_t i = 0; i < count; ++i) {
        const uint8_t* p = in.data() + 4 + (size_t)i * rec;
        uint64_t v[4];
        memcpy(v, p + 8, 32);
        std::unique_ptr<dbg_column[]> cols(new dbg_column[2]);
        memset(cols.get(), 0, 2 * sizeof(dbg_column));
        cols[0].dt.type = p[1], cols[0].dt.precision = p[2], cols[0].dt.scale = p[3];
        cols[1].dt.type = p[4], cols[1].dt.precision = p[5], cols[1].dt.scale = p[6];
        std::unique_ptr<dbg_expr_node[]> nodes(new dbg_expr_node[4]);
        memset(nodes.get(), 0, 4 * sizeof(dbg_expr_node));
        nodes[0].op = DBG_EXPR_COLUMN, nodes[0].index = 0;
        nodes[1].op = DBG_EXPR_COLUMN, nodes[1].index = 1;
        nodes[2].op = p[0] < 3 ? ops[p[0]] : 99;
        nodes[3].op = DBG_EXPR_STORE, nodes[3].index = 0;
        dbg_expr_program prog;
        memset(&prog, 0, sizeof(prog));
        prog.nodes = nodes.get(), prog.n_nodes = 4, prog.cols = cols.get(), prog.n_cols = 2, prog.n_outputs = 1;
        ExprCompiled C;
        std::string msg;
        const int rc = expr_compile(&prog, C, msg);
        if (rc != DBG_OK) {
            fprintf(out, "%d 0 0 0 0 0 0\n", rc);
            continue;
        }
        const ENode& n = C.nodes[2];
        const dbg_datatype t = C.out_types[0];
        bool err = false;
        EU128 r{0, 0};
        if (n.op == EX_NUM) {
            r.lo = expr_num(n, v[0], v[2]);
        } else if (n.op == EX_DADD) {
            r = expr_dec_add(n, EU128{v[0], v[1]}, EU128{v[2], v[3]}, &err);
        } else {
            r = expr_dec_mul(n, EU128{v[0], v[1]}, EU128{v[2], v[3]}, &err);
        }
        fprintf(out, "0 %d %d %d %llx %llx %d\n", t.type, t.precision, t.scale, (unsigned long long)r.lo, (unsigned long long)r.hi, err ? 1 : 0);
    }
    fclose(out);
    return 0;
}
