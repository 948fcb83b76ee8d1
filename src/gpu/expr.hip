// Fused expression evaluation: one launch evaluates a whole typed, null-aware
// expression program over the rows of a frame.
//
// Reference parity: cudf's compute_column (AST evaluation) as the reference's
// project and filter execs use it - SURVEY.md L0.
//
// The program (expr.hpp) is a postfix list of fixed-size instructions passed
// BY VALUE in the kernel arguments, with the tables of input columns, outputs
// and constant arrays: no copy to the device and no sync, so a call can be
// captured. The host types every instruction; the kernel never looks at a
// type at run time beyond the kind fields of the instruction it decodes.
//
// How it works:
//  * UNIFORM DISPATCH. The program counter, the stack pointer and every
//    decoded field are the same in all lanes: they live in scalar registers,
//    the instruction is fetched from the kernel argument segment with a
//    scalar load, and the dispatch switch is a scalar branch. Lanes differ
//    only in the row they hold.
//  * THE STACK IS IN LDS. stack[slot][row of the thread][thread] in 8-byte
//    entries: the slot index is scalar, so the address is
//    (slot * ROWS + r) * 2048 + tid * 8 and a wave touches 64 consecutive
//    entries - no bank conflict and no scratch, where a run-time-indexed
//    per-lane array would go. The top of the stack is cached in registers.
//    A thread only ever touches its own entries: no barrier.
//  * VALIDITY is one bit per slot in one register per row; data operations
//    ignore it (the data under a null is what the same arithmetic gives on
//    the bytes stored there).
//  * NO ATOMICS, no waits between workgroups, nothing read back.
//
// MI355X notes: the kernel is templated on the stack depth (4, 8 or 16 slots
// -> 16, 32 or 64 KiB of LDS) so that shallow programs, nearly all of them,
// keep several workgroups per CU; each thread carries EXPR_ROWS_PER_THREAD
// rows through one instruction decode to amortise the scalar work.
#include "srj_common.hpp"
#include "expr.hpp"

namespace srj {

namespace {

constexpr int ROWS = EXPR_ROWS_PER_THREAD;
static_assert(EXPR_MAX_GRID == MAX_GRID, "exported grid cap");
static_assert(EXPR_MAX_DEPTH <= 32, "validity is one bit per slot in 32 bits");

__device__ __forceinline__ double as_f64(int64_t x) {
  return __longlong_as_double(x);
}
__device__ __forceinline__ int64_t as_i64(double d) {
  return __double_as_longlong(d);
}
__device__ __forceinline__ bool is_float(int k) { return k >= EK_F32; }

// Wrap and sign-extend an integer result at the width of its kind.
__device__ __forceinline__ int64_t narrow_int(int kind, int64_t x) {
  switch (kind) {
    case EK_BOOL: return x != 0;
    case EK_I8: return (int8_t)x;
    case EK_I16: return (int16_t)x;
    case EK_I32: return (int32_t)x;
    default: return x;
  }
}

__device__ __forceinline__ double narrow_float(int kind, double d) {
  return kind == EK_F32 ? (double)(float)d : d;
}

// The slot of a value of kind `from` converted to kind `to`, as torch's
// Tensor.to does it.
__device__ __forceinline__ int64_t cast_slot(int to, int from, int64_t x) {
  if (is_float(to)) {
    if (is_float(from)) return as_i64(narrow_float(to, as_f64(x)));
    return as_i64(to == EK_F32 ? (double)(float)x : (double)x);
  }
  if (is_float(from)) {
    const double d = as_f64(x);
    if (to == EK_BOOL) return d != 0.0;
    return narrow_int(to, (int64_t)d);
  }
  return narrow_int(to, x);
}

__device__ __forceinline__ bool truthy(int kind, int64_t x) {
  return is_float(kind) ? as_f64(x) != 0.0 : x != 0;
}

// The slots of ROWS rows of a column. The kind switch is outside the row
// loop and nothing is conditional on the lane, so the loads of all rows are
// issued back to back and waited for once.
template <typename T>
__device__ __forceinline__ void load_rows(const void* p,
                                          const int64_t (&at)[EXPR_ROWS_PER_THREAD],
                                          int64_t (&x)[EXPR_ROWS_PER_THREAD]) {
#pragma unroll
  for (int r = 0; r < EXPR_ROWS_PER_THREAD; ++r)
    x[r] = static_cast<const T*>(p)[at[r]];
}

__device__ __forceinline__ void load_slots(
    const void* p, int kind, const int64_t (&at)[EXPR_ROWS_PER_THREAD],
    int64_t (&x)[EXPR_ROWS_PER_THREAD]) {
  switch (kind) {
    case EK_BOOL:
      load_rows<uint8_t>(p, at, x);
#pragma unroll
      for (int r = 0; r < EXPR_ROWS_PER_THREAD; ++r) x[r] = x[r] != 0;
      break;
    case EK_I8: load_rows<int8_t>(p, at, x); break;
    case EK_I16: load_rows<int16_t>(p, at, x); break;
    case EK_I32: load_rows<int32_t>(p, at, x); break;
    case EK_F32: {
      float f[EXPR_ROWS_PER_THREAD];
#pragma unroll
      for (int r = 0; r < EXPR_ROWS_PER_THREAD; ++r)
        f[r] = static_cast<const float*>(p)[at[r]];
#pragma unroll
      for (int r = 0; r < EXPR_ROWS_PER_THREAD; ++r)
        x[r] = as_i64((double)f[r]);
      break;
    }
    default: load_rows<int64_t>(p, at, x); break;
  }
}

__device__ __forceinline__ void store_slot(void* p, int kind, int64_t row,
                                           int64_t x) {
  switch (kind) {
    case EK_BOOL: static_cast<uint8_t*>(p)[row] = x != 0; break;
    case EK_I8: static_cast<int8_t*>(p)[row] = (int8_t)x; break;
    case EK_I16: static_cast<int16_t*>(p)[row] = (int16_t)x; break;
    case EK_I32: static_cast<int32_t*>(p)[row] = (int32_t)x; break;
    case EK_F32: static_cast<float*>(p)[row] = (float)as_f64(x); break;
    default: static_cast<int64_t*>(p)[row] = x; break;
  }
}

__device__ __forceinline__ int64_t arith(int op, int kind, int64_t a,
                                         int64_t b) {
  if (is_float(kind)) {
    const double x = as_f64(a), y = as_f64(b);
    const double r = op == EO_ADD ? x + y : op == EO_SUB ? x - y : x * y;
    return as_i64(narrow_float(kind, r));
  }
  const uint64_t x = (uint64_t)a, y = (uint64_t)b;
  const uint64_t r = op == EO_ADD ? x + y : op == EO_SUB ? x - y : x * y;
  return narrow_int(kind, (int64_t)r);
}

__device__ __forceinline__ bool compare(int op, int kind, int64_t a,
                                        int64_t b) {
  if (is_float(kind)) {
    const double x = as_f64(a), y = as_f64(b);
    switch (op) {
      case EO_EQ: return x == y;
      case EO_NE: return x != y;
      case EO_LT: return x < y;
      case EO_LE: return x <= y;
      case EO_GT: return x > y;
      default: return x >= y;
    }
  }
  switch (op) {
    case EO_EQ: return a == b;
    case EO_NE: return a != b;
    case EO_LT: return a < b;
    case EO_LE: return a <= b;
    case EO_GT: return a > b;
    default: return a >= b;
  }
}

// Membership of x in the sorted array set[0, len): a fixed number of steps
// for a given len, so the loop is uniform.
__device__ __forceinline__ bool in_sorted(const int64_t* set, int64_t len,
                                          int64_t x) {
  if (len <= 0) return false;
  int64_t lo = 0, n = len;
  while (n > 1) {
    const int64_t half = n >> 1;
    if (set[lo + half] <= x) lo += half;
    n -= half;
  }
  return set[lo] == x;
}

template <int DEPTH>
__global__ __launch_bounds__(DEFAULT_BLOCK) void expr_eval_kernel(
    const ExprProgram prog, const int64_t rows) {
  __shared__ int64_t stack[DEPTH][ROWS][DEFAULT_BLOCK];
  const int tid = threadIdx.x;
  const int64_t pass = (int64_t)gridDim.x * DEFAULT_BLOCK * ROWS;
  for (int64_t base = (int64_t)blockIdx.x * DEFAULT_BLOCK * ROWS; base < rows;
       base += pass) {
    int64_t row[ROWS];
    int64_t at[ROWS];  // the row to load: dead lanes read the last row
    bool live[ROWS];
    int64_t top[ROWS];    // slot sp - 1
    uint32_t vbits[ROWS];  // bit s: slot s is valid
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      row[r] = base + (int64_t)r * DEFAULT_BLOCK + tid;
      live[r] = row[r] < rows;
      at[r] = live[r] ? row[r] : rows - 1;
      top[r] = 0;
      vbits[r] = 0;
    }
    int sp = 0;
    const int n = prog.ninstrs;
    for (int pc = 0; pc < n; ++pc) {
      const ExprInstr ins = prog.instrs[pc];
      const int op = ins.op;
      const int kind = ins.kind;
      const int ka = ins.arg & 15, kb = (ins.arg >> 4) & 15;
      switch (op) {
        case EO_LOAD_COL:
        case EO_LIT: {
          // push: the cached top moves to its LDS slot
          if (sp > 0) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) stack[sp - 1][r][tid] = top[r];
          }
          if (op == EO_LIT) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
              top[r] = ins.imm;
              vbits[r] = ins.arg ? vbits[r] & ~(1u << sp) : vbits[r] | (1u << sp);
            }
          } else {
            const ExprInput in = prog.inputs[ins.arg];
            uint8_t v[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
              v[r] = in.valid != nullptr ? in.valid[at[r]] : 1;
            load_slots(in.data, in.kind, at, top);
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
              vbits[r] = v[r] ? vbits[r] | (1u << sp) : vbits[r] & ~(1u << sp);
          }
          ++sp;
          break;
        }
        case EO_ADD: case EO_SUB: case EO_MUL: case EO_DIV:
        case EO_EQ: case EO_NE: case EO_LT: case EO_LE: case EO_GT:
        case EO_GE: case EO_AND: case EO_OR: case EO_COALESCE_STEP: {
          // [a, b] -> one value in slot sp - 2
          const uint32_t abit = 1u << (sp - 2);
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
            const int64_t a = stack[sp - 2][r][tid];
            const int64_t b = top[r];
            const bool av = (vbits[r] >> (sp - 2)) & 1;
            const bool bv = (vbits[r] >> (sp - 1)) & 1;
            int64_t res;
            bool rv = av && bv;
            if (op <= EO_MUL) {
              res = arith(op, kind, cast_slot(kind, ka, a),
                          cast_slot(kind, kb, b));
            } else if (op == EO_DIV) {
              const double x = as_f64(cast_slot(EK_F64, ka, a));
              const double y = as_f64(cast_slot(EK_F64, kb, b));
              const bool zero = y == 0.0;
              res = as_i64(x / (zero ? 1.0 : y));
              rv = rv && !zero;
            } else if (op <= EO_GE) {
              res = compare(op, kind, cast_slot(kind, ka, a),
                            cast_slot(kind, kb, b));
            } else if (op == EO_AND) {
              const bool x = truthy(ka, a), y = truthy(kb, b);
              rv = (av && bv) || (av && !x) || (bv && !y);
              res = x && y && rv;
            } else if (op == EO_OR) {
              const bool x = truthy(ka, a), y = truthy(kb, b);
              rv = (av && bv) || (av && x) || (bv && y);
              res = x || y;
            } else {
              res = av ? cast_slot(kind, ka, a) : cast_slot(kind, kb, b);
              rv = av || bv;
            }
            top[r] = res;
            vbits[r] = rv ? vbits[r] | abit : vbits[r] & ~abit;
          }
          --sp;
          break;
        }
        case EO_NOT:
#pragma unroll
          for (int r = 0; r < ROWS; ++r) top[r] = !truthy(ka, top[r]);
          break;
        case EO_IS_NULL:
        case EO_IS_NOT_NULL:
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
            const bool v = (vbits[r] >> (sp - 1)) & 1;
            top[r] = (op == EO_IS_NULL) ? !v : v;
            vbits[r] |= 1u << (sp - 1);
          }
          break;
        case EO_ABS:
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
            if (is_float(kind)) {
              top[r] = top[r] & 0x7fffffffffffffffLL;
            } else {
              const uint64_t u = (uint64_t)top[r];
              top[r] = narrow_int(kind, (int64_t)(top[r] < 0 ? 0 - u : u));
            }
          }
          break;
        case EO_CAST:
#pragma unroll
          for (int r = 0; r < ROWS; ++r) top[r] = cast_slot(kind, ka, top[r]);
          break;
        case EO_IN_SET: {
          const ExprConst c = prog.consts[ins.imm];
#pragma unroll
          for (int r = 0; r < ROWS; ++r)
            top[r] = in_sorted(c.data, c.len, top[r]);
          break;
        }
        case EO_LUT: {
          const ExprConst c = prog.consts[ins.imm];
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
            int64_t i = top[r];
            i = i < 0 ? 0 : (i >= c.len ? c.len - 1 : i);
            top[r] = narrow_int(kind, c.data[i]);
          }
          break;
        }
        case EO_SELECT: {
          // [running, value, cond] -> slot sp - 3
          const uint32_t obit = 1u << (sp - 3);
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
            const bool hit = truthy(ka, top[r]) && ((vbits[r] >> (sp - 1)) & 1);
            const int s = hit ? sp - 2 : sp - 3;
            const int64_t value = stack[sp - 2][r][tid];
            const int64_t running = stack[sp - 3][r][tid];
            const bool v = (vbits[r] >> s) & 1;
            top[r] = hit ? value : running;
            vbits[r] = v ? vbits[r] | obit : vbits[r] & ~obit;
          }
          sp -= 2;
          break;
        }
        case EO_STORE:
        case EO_STORE_KEEP: {
          const ExprOutput out = prog.outputs[ins.arg];
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
            if (!live[r]) continue;
            const bool v = (vbits[r] >> (sp - 1)) & 1;
            if (op == EO_STORE_KEEP) {
              static_cast<uint8_t*>(out.data)[row[r]] = truthy(kind, top[r]) && v;
            } else {
              store_slot(out.data, kind, row[r], top[r]);
              if (out.valid != nullptr) out.valid[row[r]] = v;
            }
          }
          --sp;
          if (sp > 0) {
#pragma unroll
            for (int r = 0; r < ROWS; ++r) top[r] = stack[sp - 1][r][tid];
          }
          break;
        }
        default:
          break;
      }
    }
  }
}

}  // namespace

}  // namespace srj

// The binding has validated the program (bind_expr.cpp): every index is in
// range and the stack stays within [0, depth], depth <= EXPR_MAX_DEPTH.
extern "C" void srj_expr_eval(const srj::ExprProgram* prog, int32_t depth,
                              int64_t rows, hipStream_t stream) {
  using namespace srj;
  if (rows <= 0) return;
  const int64_t per_block = (int64_t)DEFAULT_BLOCK * EXPR_ROWS_PER_THREAD;
  const dim3 grid((unsigned)grid_1d((rows + per_block - 1) / per_block *
                                    DEFAULT_BLOCK));
  const dim3 block(DEFAULT_BLOCK);
  if (depth <= 4)
    expr_eval_kernel<4><<<grid, block, 0, stream>>>(*prog, rows);
  else if (depth <= 8)
    expr_eval_kernel<8><<<grid, block, 0, stream>>>(*prog, rows);
  else
    expr_eval_kernel<16><<<grid, block, 0, stream>>>(*prog, rows);
}
