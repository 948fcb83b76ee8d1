// Fused expression evaluation: the program format shared by expr.hip and
// bind_expr.cpp. Python mirrors the numeric values in ops/expr.py.
#pragma once
#include <cstdint>

namespace srj {

// Element kinds. A stack slot is 64 bits: the integer kinds (and BOOL as 0/1)
// sit sign-extended in an int64, F32 and F64 as the bits of a double (every
// float is a double, and +, -, * and / in double followed by one rounding to
// float equal the float operation).
enum ExprKind : int32_t {
  EK_BOOL = 0,
  EK_I8 = 1,
  EK_I16 = 2,
  EK_I32 = 3,
  EK_I64 = 4,
  EK_F32 = 5,
  EK_F64 = 6,
  EK_COUNT = 7,
};

// `kind` is the result kind unless noted; `arg` of the two-operand ops holds
// the operand kinds as (left | right << 4), of the one-operand ops the
// operand kind.
enum ExprOp : int32_t {
  EO_LOAD_COL = 0,   // arg = input
  EO_LIT = 1,        // imm = value bits (int64 or double); arg = 1: null
  EO_ADD = 2,
  EO_SUB = 3,
  EO_MUL = 4,
  EO_DIV = 5,        // F64; divisor 0 -> 1, result null
  EO_EQ = 6,         // comparisons: kind = the common operand kind
  EO_NE = 7,
  EO_LT = 8,
  EO_LE = 9,
  EO_GT = 10,
  EO_GE = 11,
  EO_AND = 12,       // Kleene; data masked by validity
  EO_OR = 13,        // Kleene; data not masked
  EO_NOT = 14,
  EO_IS_NULL = 15,
  EO_IS_NOT_NULL = 16,
  EO_ABS = 17,
  EO_CAST = 18,      // arg = from kind
  EO_IN_SET = 19,    // imm = constant array; arg = operand kind (integer)
  EO_LUT = 20,       // imm = constant array; table[clamp(value)]
  EO_SELECT = 21,    // [running, value, cond] -> cond ? value : running
  EO_COALESCE_STEP = 22,  // [running, next] -> running valid ? running : next
  EO_STORE = 23,     // arg = output; kind = the output's element kind
  EO_STORE_KEEP = 24,  // arg = output; kind = operand kind; one byte:
                       // data != 0 && valid
  EO_COUNT = 25,
};

struct ExprInstr {
  uint8_t op;
  uint8_t kind;
  uint16_t arg;
  uint32_t reserved;
  int64_t imm;
};
static_assert(sizeof(ExprInstr) == 16, "instruction size");

struct ExprInput {
  const void* data;
  const uint8_t* valid;  // byte per row, zero = null; may be null
  int32_t kind;
  int32_t reserved;
};

struct ExprOutput {
  void* data;
  uint8_t* valid;  // byte per row; may be null
};

struct ExprConst {
  const int64_t* data;
  int64_t len;
};

constexpr int EXPR_MAX_INSTRS = 160;
constexpr int EXPR_MAX_DEPTH = 16;
constexpr int EXPR_MAX_INPUTS = 24;
constexpr int EXPR_MAX_OUTPUTS = 8;
constexpr int EXPR_MAX_CONSTS = 16;
constexpr int EXPR_ROWS_PER_THREAD = 2;
// the project's grid cap (srj_common.hpp MAX_GRID; expr.hip asserts it): one
// grid pass covers EXPR_MAX_GRID * 256 * EXPR_ROWS_PER_THREAD rows
constexpr int EXPR_MAX_GRID = 2048;

// Passed to the kernel by value: no copy to the device, no sync.
struct ExprProgram {
  int32_t ninstrs;
  int32_t ninputs;
  int32_t noutputs;
  int32_t nconsts;
  ExprInstr instrs[EXPR_MAX_INSTRS];
  ExprInput inputs[EXPR_MAX_INPUTS];
  ExprOutput outputs[EXPR_MAX_OUTPUTS];
  ExprConst consts[EXPR_MAX_CONSTS];
};
static_assert(sizeof(ExprProgram) <= 3968, "kernel arguments are 4 KiB");

}  // namespace srj
