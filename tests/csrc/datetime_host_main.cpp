// datetime_host_main.cpp — the host build of the date / time functions and of length()'s byte rule
// (databend_amd/csrc/expr.hpp: expr_compile, expr_civil, expr_func, expr_char_starts) as a program
// of its own, for a run under -fsanitize=address,undefined (tests/test_datetime_host.py).  Nothing
// here is loaded into Python.
//
//   datetime_host_main <cases.bin> <out.txt>
//
// cases.bin: u32 count, then per case 16 bytes
//   u8 kind, u8 func (a dbg_expr_func), u8 type (DBG_DATE / DBG_TIMESTAMP), u8 nullable, u32 pad, i64 value
//   kind 0: the program [COLUMN 0, FUNC func, STORE 0]
//   kind 1: the program to_year(c) * 100 + to_month(c)  ([COLUMN 0, FUNC, CONST 100_u8, MULTIPLY, COLUMN 0, FUNC, PLUS, STORE 0])
//   kind 2: length: `value` bytes follow the record, padded to a multiple of 4; the bytes are counted
//           a word at a time with expr_char_starts, as the kernel counts a chunk
// Each program goes through expr_compile and its lowered nodes are run over a plain vector stack with
// the per-row operators the kernel calls.  out.txt, one line per case:
//   "<status> <type> <nullable> <value hex>"      (status != 0: the rest is zeros)
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

static uint64_t run_nodes(const ExprCompiled& C, uint64_t cell) {
    std::vector<uint64_t> st;
    uint64_t stored = 0;
    for (const ENode& n : C.nodes) {
        if (n.op == EX_COL) {
            st.push_back(cell);
        } else if (n.op == EX_CONST) {
            st.push_back(n.c[0]);
        } else if (n.op == EX_STORE) {
            stored = st.back();
            if (n.flags & EX_F_POP) st.pop_back();
        } else if (n.op == EX_FUNC) {
            st.back() = expr_func(n, st.back());
        } else if (n.op == EX_NUM) {
            const uint64_t b = st.back();
            st.pop_back();
            const uint64_t a = st.back();
            st.pop_back();
            st.push_back(expr_num(n, a, b));
        } else {
            abort();
        }
    }
    return stored;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: datetime_host_main <cases.bin> <out.txt>\n");
        return 2;
    }
    std::vector<uint8_t> in;
    if (!read_all(argv[1], in) || in.size() < 4) return 2;
    uint32_t count;
    memcpy(&count, in.data(), 4);
    FILE* out = fopen(argv[2], "w");
    if (!out) return 2;
    size_t at = 4;
    for (uint32_t i = 0; i < count; ++i) {
        if (at + 16 > in.size()) return 2;
        const uint8_t* p = in.data() + at;
        at += 16;
        int64_t value;
        memcpy(&value, p + 8, 8);
        if (p[0] == 2) {
            const size_t len = (size_t)value, padded = (len + 3) & ~(size_t)3;
            if (at + padded > in.size()) return 2;
            std::unique_ptr<uint8_t[]> bytes(new uint8_t[padded ? padded : 1]);
            memcpy(bytes.get(), &in[at], padded);
            at += padded;
            uint64_t n = 0;
            for (size_t k = 0; k < padded; k += 4) {
                uint32_t w;
                memcpy(&w, bytes.get() + k, 4);
                uint32_t m = expr_char_starts(w);
                if (len - k < 4) m &= (1u << (len - k)) - 1u;  // the bytes past the end are not the string's
                n += (uint64_t)__builtin_popcount(m);
            }
            fprintf(out, "0 %d 0 %llx\n", DBG_UINT64, (unsigned long long)n);
            continue;
        }
        const int n_nodes = p[0] == 0 ? 3 : 8;
        std::unique_ptr<dbg_column[]> cols(new dbg_column[1]);
        memset(cols.get(), 0, sizeof(dbg_column));
        cols[0].dt.type = p[2], cols[0].dt.nullable = p[3];
        std::unique_ptr<dbg_expr_node[]> nodes(new dbg_expr_node[n_nodes]);
        memset(nodes.get(), 0, n_nodes * sizeof(dbg_expr_node));
        if (p[0] == 0) {
            nodes[0].op = DBG_EXPR_COLUMN;
            nodes[1].op = DBG_EXPR_FUNC, nodes[1].index = p[1];
            nodes[2].op = DBG_EXPR_STORE;
        } else {
            nodes[0].op = DBG_EXPR_COLUMN;
            nodes[1].op = DBG_EXPR_FUNC, nodes[1].index = DBG_FUNC_TO_YEAR;
            nodes[2].op = DBG_EXPR_CONST, nodes[2].dt.type = DBG_UINT8, nodes[2].i64 = 100;
            nodes[3].op = DBG_EXPR_MULTIPLY;
            nodes[4].op = DBG_EXPR_COLUMN;
            nodes[5].op = DBG_EXPR_FUNC, nodes[5].index = DBG_FUNC_TO_MONTH;
            nodes[6].op = DBG_EXPR_PLUS;
            nodes[7].op = DBG_EXPR_STORE;
        }
        dbg_expr_program prog;
        memset(&prog, 0, sizeof(prog));
        prog.nodes = nodes.get(), prog.n_nodes = n_nodes, prog.cols = cols.get(), prog.n_cols = 1, prog.n_outputs = 1;
        ExprCompiled C;
        std::string msg;
        const int rc = expr_compile(&prog, C, msg);
        if (rc != DBG_OK) {
            fprintf(out, "%d 0 0 0\n", rc);
            continue;
        }
        // the cell as the kernel's loads leave it: a Date zero-extended from its 32 bits
        const uint64_t cell = p[2] == DBG_DATE ? (uint64_t)(uint32_t)(int32_t)value : (uint64_t)value;
        const uint64_t r = run_nodes(C, cell);
        fprintf(out, "0 %d %d %llx\n", C.out_types[0].type, C.out_types[0].nullable, (unsigned long long)r);
    }
    fclose(out);
    return at == in.size() ? 0 : 2;
}
