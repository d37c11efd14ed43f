// Stand-alone check of ew_step_check (ops/csrc/ewdml_ops.h), the validation every fused decode
// entry point runs before its launch.  Built with -fsanitize=address,undefined and run as a child
// process by tests/unit/test_step_check.py; exits 0 when every case behaves.
#include <cstdio>
#include <string>

#include "ewdml_ops.h"

static int failures = 0;

// `want` empty: the description must pass; else the exception's text must be "who: " + want
static void expect(const char* what, const StepArgs& s, bool need_mom, const std::string& want) {
  const std::string who = "ewdml test decode";
  std::string got;
  try {
    ew_step_check(who, s, need_mom);
  } catch (const std::runtime_error& e) {
    got = e.what();
  }
  const std::string full = want.empty() ? "" : who + ": " + want;
  if (got != full) {
    std::printf("FAIL %s: got \"%s\", want \"%s\"\n", what, got.c_str(), full.c_str());
    ++failures;
  } else {
    std::printf("ok   %s\n", what);
  }
}

int main() {
  // addresses only: nothing is dereferenced
  StepArgs ok{};
  ok.param = 0x10000;
  ok.mom = 0x20000;
  ok.grad_out = 0x30000;
  ok.shadow = 0x40008;  // 8-byte aligned is enough for the bf16 shadow
  ok.lr = 0.1f;
  ok.momentum = 0.9f;
  ok.grad_scale = 0.5f;
  ok.nesterov = 1;
  ok.apply = 1;
  ok.key_state = 0x50004;
  ok.lr_ptr = 0x60004;
  expect("valid step", ok, false, "");
  expect("valid step, buffer required", ok, true, "");

  StepArgs out_only{};
  out_only.grad_out = 0x30000;
  out_only.grad_scale = 1.0f;
  expect("grad_out only", out_only, true, "");

  StepArgs plain = ok;  // a step without momentum needs no buffer
  plain.mom = 0;
  plain.momentum = 0.0f;
  plain.nesterov = 0;
  expect("no momentum, no buffer", plain, false, "");

  StepArgs s = ok;
  s.param = 0;
  expect("apply without parameters", s, false, "apply needs the parameters");

  s = StepArgs{};
  expect("neither apply nor grad_out", s, false, "nothing to write");

  s = plain;
  s.momentum = 0.9f;
  expect("momentum without a buffer", s, false, "a momentum step needs the momentum buffer");

  s = plain;
  s.nesterov = 1;
  expect("nesterov without a buffer", s, false, "a momentum step needs the momentum buffer");

  expect("need_mom without a buffer", plain, true, "a momentum step needs the momentum buffer");

  s = ok;
  s.param += 4;
  expect("param + 4 bytes", s, false, "misaligned operand");

  s = ok;
  s.shadow += 2;
  expect("shadow + 2 bytes", s, false, "misaligned operand");

  s = ok;
  s.lr_ptr += 1;
  expect("lr_ptr + 1 byte", s, false, "misaligned operand");

  if (failures) std::printf("%d case(s) failed\n", failures);
  return failures ? 1 : 0;
}
