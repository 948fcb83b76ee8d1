// Bindings for the fused expression kernel.
#include "srj_bind.hpp"
#include "expr.hpp"

#include <cstring>
#include <tuple>
#include <vector>

using srj::ExprProgram;

extern "C" void srj_expr_eval(const ExprProgram*, int32_t, int64_t,
                              hipStream_t);

namespace {

// (data, valid, kind)
using Input = std::tuple<uintptr_t, uintptr_t, int32_t>;
// (data, valid)
using Output = std::tuple<uintptr_t, uintptr_t>;
// (data, len)
using Const = std::tuple<uintptr_t, int64_t>;

int kind_width(int k) {
  switch (k) {
    case srj::EK_BOOL: case srj::EK_I8: return 1;
    case srj::EK_I16: return 2;
    case srj::EK_I32: case srj::EK_F32: return 4;
    default: return 8;
  }
}

bool known_kind(int k) { return k >= 0 && k < srj::EK_COUNT; }
bool int_kind(int k) { return k >= srj::EK_BOOL && k <= srj::EK_I64; }

// Fills `p` from the Python-side tables, checks every field the kernel
// trusts and dry-runs the program. Returns the deepest stack.
int build_program(ExprProgram& p, const std::string& code,
                  const std::vector<Input>& inputs,
                  const std::vector<Output>& outputs,
                  const std::vector<Const>& consts) {
  using namespace srj;
  if (code.size() % sizeof(ExprInstr) != 0)
    throw std::invalid_argument("expr: program is not a whole number of "
                                "instructions");
  const size_t n = code.size() / sizeof(ExprInstr);
  if (n == 0) throw std::invalid_argument("expr: empty program");
  if (n > (size_t)EXPR_MAX_INSTRS)
    throw std::invalid_argument("expr: more than EXPR_MAX_INSTRS instructions");
  if (inputs.size() > (size_t)EXPR_MAX_INPUTS)
    throw std::invalid_argument("expr: more than EXPR_MAX_INPUTS inputs");
  if (outputs.empty() || outputs.size() > (size_t)EXPR_MAX_OUTPUTS)
    throw std::invalid_argument("expr: 1..EXPR_MAX_OUTPUTS outputs per call");
  if (consts.size() > (size_t)EXPR_MAX_CONSTS)
    throw std::invalid_argument("expr: more than EXPR_MAX_CONSTS constant "
                                "arrays");
  std::memset(&p, 0, sizeof(p));
  p.ninstrs = (int32_t)n;
  p.ninputs = (int32_t)inputs.size();
  p.noutputs = (int32_t)outputs.size();
  p.nconsts = (int32_t)consts.size();
  std::memcpy(p.instrs, code.data(), code.size());
  for (size_t i = 0; i < inputs.size(); ++i) {
    const std::string w = "expr: inputs[" + std::to_string(i) + "]";
    const int k = std::get<2>(inputs[i]);
    if (!known_kind(k)) throw std::invalid_argument(w + ": unknown kind");
    if (std::get<0>(inputs[i]) == 0)
      throw std::invalid_argument(w + ": null data");
    if (std::get<0>(inputs[i]) % kind_width(k) != 0)
      throw std::invalid_argument(w + ": data not aligned to its element");
    p.inputs[i].data = as_ptr<const void>(std::get<0>(inputs[i]));
    p.inputs[i].valid = as_ptr<const uint8_t>(std::get<1>(inputs[i]));
    p.inputs[i].kind = k;
  }
  for (size_t i = 0; i < consts.size(); ++i) {
    const std::string w = "expr: consts[" + std::to_string(i) + "]";
    const int64_t len = std::get<1>(consts[i]);
    if (len < 0) throw std::invalid_argument(w + ": negative length");
    if (len > 0 && std::get<0>(consts[i]) == 0)
      throw std::invalid_argument(w + ": null data");
    if (std::get<0>(consts[i]) % 8 != 0)
      throw std::invalid_argument(w + ": data not aligned to 8 bytes");
    p.consts[i].data = as_ptr<const int64_t>(std::get<0>(consts[i]));
    p.consts[i].len = len;
  }
  for (size_t i = 0; i < outputs.size(); ++i) {
    if (std::get<0>(outputs[i]) == 0)
      throw std::invalid_argument("expr: outputs[" + std::to_string(i) +
                                  "]: null data");
    p.outputs[i].data = as_ptr<void>(std::get<0>(outputs[i]));
    p.outputs[i].valid = as_ptr<uint8_t>(std::get<1>(outputs[i]));
  }

  // dry run: stack depth, operand counts, indices
  std::vector<bool> stored(outputs.size(), false);
  int sp = 0, deepest = 0;
  for (size_t pc = 0; pc < n; ++pc) {
    const ExprInstr& in = p.instrs[pc];
    const std::string w = "expr: instrs[" + std::to_string(pc) + "]";
    if (in.op >= EO_COUNT) throw std::invalid_argument(w + ": unknown op");
    if (!known_kind(in.kind)) throw std::invalid_argument(w + ": unknown kind");
    const int ka = in.arg & 15, kb = (in.arg >> 4) & 15;
    int pops = 0, pushes = 0;
    bool two_kinds = false, one_kind = false;
    switch (in.op) {
      case EO_LOAD_COL:
        if (in.arg >= inputs.size())
          throw std::invalid_argument(w + ": input out of range");
        pushes = 1;
        break;
      case EO_LIT:
        if (in.arg > 1) throw std::invalid_argument(w + ": arg must be 0 or 1");
        pushes = 1;
        break;
      case EO_SUB:
        if (in.kind == EK_BOOL)
          throw std::invalid_argument(w + ": BOOL subtraction");
        [[fallthrough]];
      case EO_ADD: case EO_MUL: case EO_EQ: case EO_NE: case EO_LT:
      case EO_LE: case EO_GT: case EO_GE: case EO_AND: case EO_OR:
      case EO_COALESCE_STEP:
        pops = 2; pushes = 1; two_kinds = true;
        break;
      case EO_DIV:
        if (in.kind != EK_F64)
          throw std::invalid_argument(w + ": DIV is F64");
        pops = 2; pushes = 1; two_kinds = true;
        break;
      case EO_NOT: case EO_CAST:
        pops = 1; pushes = 1; one_kind = true;
        break;
      case EO_IS_NULL: case EO_IS_NOT_NULL:
        pops = 1; pushes = 1;
        break;
      case EO_ABS:
        if (in.kind == EK_BOOL) throw std::invalid_argument(w + ": BOOL ABS");
        pops = 1; pushes = 1;
        break;
      case EO_IN_SET: case EO_LUT:
        if (in.imm < 0 || in.imm >= (int64_t)consts.size())
          throw std::invalid_argument(w + ": constant array out of range");
        if (in.op == EO_LUT && p.consts[in.imm].len < 1)
          throw std::invalid_argument(w + ": empty lookup table");
        if (in.op == EO_LUT && !int_kind(in.kind))
          throw std::invalid_argument(w + ": LUT kind must be an integer");
        if (!int_kind(ka) || in.arg > 15)
          throw std::invalid_argument(w + ": operand must be an integer");
        pops = 1; pushes = 1;
        break;
      case EO_SELECT:
        pops = 3; pushes = 1; one_kind = true;
        break;
      case EO_STORE: case EO_STORE_KEEP: {
        if (in.arg >= outputs.size())
          throw std::invalid_argument(w + ": output out of range");
        const size_t k = in.arg;
        if (stored[k])
          throw std::invalid_argument(w + ": output stored twice");
        stored[k] = true;
        const int width = in.op == EO_STORE ? kind_width(in.kind) : 1;
        if (std::get<0>(outputs[k]) % width != 0)
          throw std::invalid_argument(w + ": output not aligned to its "
                                      "element");
        pops = 1;
        break;
      }
      default:
        break;
    }
    if (two_kinds && (!known_kind(ka) || !known_kind(kb) || in.arg > 255))
      throw std::invalid_argument(w + ": unknown operand kind");
    if (one_kind && (!known_kind(ka) || in.arg > 15))
      throw std::invalid_argument(w + ": unknown operand kind");
    if (sp < pops) throw std::invalid_argument(w + ": stack underflow");
    sp += pushes - pops;
    if (sp > EXPR_MAX_DEPTH)
      throw std::invalid_argument(w + ": stack deeper than EXPR_MAX_DEPTH");
    if (sp > deepest) deepest = sp;
  }
  if (sp != 0)
    throw std::invalid_argument("expr: values left on the stack");
  for (size_t i = 0; i < stored.size(); ++i)
    if (!stored[i])
      throw std::invalid_argument("expr: outputs[" + std::to_string(i) +
                                  "] is never stored");
  return deepest;
}

}  // namespace

void register_expr(py::module_& m) {
  m.attr("EXPR_MAX_INSTRS") = srj::EXPR_MAX_INSTRS;
  m.attr("EXPR_MAX_DEPTH") = srj::EXPR_MAX_DEPTH;
  m.attr("EXPR_MAX_INPUTS") = srj::EXPR_MAX_INPUTS;
  m.attr("EXPR_MAX_OUTPUTS") = srj::EXPR_MAX_OUTPUTS;
  m.attr("EXPR_MAX_CONSTS") = srj::EXPR_MAX_CONSTS;
  m.attr("EXPR_ROWS_PER_THREAD") = srj::EXPR_ROWS_PER_THREAD;
  m.attr("EXPR_MAX_GRID") = srj::EXPR_MAX_GRID;
  // Validates like expr_eval and returns the deepest stack, without a launch.
  m.def("expr_check",
        [](const py::bytes& code, const std::vector<Input>& inputs,
           const std::vector<Output>& outputs,
           const std::vector<Const>& consts, int64_t rows) {
          if (rows < 0) throw std::invalid_argument("expr: rows < 0");
          ExprProgram p;
          return build_program(p, code, inputs, outputs, consts);
        });
  m.def("expr_eval",
        [](const py::bytes& code, const std::vector<Input>& inputs,
           const std::vector<Output>& outputs,
           const std::vector<Const>& consts, int64_t rows, uintptr_t stream) {
          if (rows < 0) throw std::invalid_argument("expr: rows < 0");
          ExprProgram p;
          const int depth = build_program(p, code, inputs, outputs, consts);
          if (rows == 0) return;
          srj_expr_eval(&p, depth, rows, as_stream(stream));
          check_hip("expr_eval");
        });
}
