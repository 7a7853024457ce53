// go2nn_trace.h — the trajectory recorder's frame kernel (include/go2nn.h: go2nn_trace_*, added within ABI 7; go2_rl_gym_amd/utils/recorder.py).
// Included at the end of go2nn_impl.cpp after go2nn_eval.h (FAIL, HIPCHK are the former's helpers; EVAL_FN, eval_f, eval_b the latter's).
//
// go2nn_trace_record: one launch per env step, one lane per OUTPUT float: lane i writes column c = i % WIDTH of tracked robot k = i / WIDTH, so a frame row (448 bytes) and
// with it the whole slot [K, WIDTH] is written densely, 256 bytes per wave store.  The reads are the scattered side — one float per lane from one of thirteen buffers, found
// by the column's block — and they are small: 112 floats per tracked robot, a few robots.  The slot is (*cursor) % T with the cursor read from device memory (every lane reads
// the same address: one broadcast load), and the cursor is advanced by a second, one-lane launch on the same stream, i.e. after every lane of the frame kernel has read it:
// no atomics, no fences between workgroups, and a captured pair lands in the next slot on every replay.  The host build runs the same element function in plain loops.
#ifndef GO2NN_TRACE_H
#define GO2NN_TRACE_H

#define TRACE_THREADS 256

// column c of env e's frame: the table of include/go2nn.h
EVAL_FN float trace_value(const Go2nnTraceIn& in, int e, int c) {
  if (c < GO2NN_TRACE_DOF_POS) return eval_f(in.root_states, e, c);
  if (c < GO2NN_TRACE_TORQUES) {
    const int vel = c >= GO2NN_TRACE_DOF_VEL, j = c - (vel ? GO2NN_TRACE_DOF_VEL : GO2NN_TRACE_DOF_POS);
    return ((const float*)in.dof_state.p)[(long long)e * in.dof_state.env_stride + (long long)j * in.dof_state.comp_stride + (vel ? in.dof_vel_offset : 0)];
  }
  if (c < GO2NN_TRACE_ACTIONS) return eval_f(in.torques, e, c - GO2NN_TRACE_TORQUES);
  if (c < GO2NN_TRACE_COMMANDS) return eval_f(in.actions, e, c - GO2NN_TRACE_ACTIONS);
  if (c < GO2NN_TRACE_BASE_LIN_VEL) return eval_f(in.commands, e, c - GO2NN_TRACE_COMMANDS);
  if (c < GO2NN_TRACE_BASE_ANG_VEL) return eval_f(in.base_lin_vel, e, c - GO2NN_TRACE_BASE_LIN_VEL);
  if (c < GO2NN_TRACE_PROJECTED_GRAVITY) return eval_f(in.base_ang_vel, e, c - GO2NN_TRACE_BASE_ANG_VEL);
  if (c < GO2NN_TRACE_FOOT_POS) return eval_f(in.projected_gravity, e, c - GO2NN_TRACE_PROJECTED_GRAVITY);
  if (c < GO2NN_TRACE_FOOT_FORCE) {          // rigid_body_states[foot, 0:3] (position) or [foot, 7:10] (linear velocity)
    const int vel = c >= GO2NN_TRACE_FOOT_VEL, r = c - (vel ? GO2NN_TRACE_FOOT_VEL : GO2NN_TRACE_FOOT_POS);
    const Go2nnEvalField& f = in.rigid_body_states;
    return ((const float*)f.p)[(long long)e * f.env_stride + (long long)in.foot_body[r / 3] * in.rigid_body_stride + (long long)(r % 3 + (vel ? 7 : 0)) * f.comp_stride];
  }
  if (c < GO2NN_TRACE_REWARD) {
    const int r = c - GO2NN_TRACE_FOOT_FORCE;
    const Go2nnEvalField& f = in.contact_forces;
    return ((const float*)f.p)[(long long)e * f.env_stride + (long long)in.foot_body[r / 3] * in.contact_body_stride + (long long)(r % 3) * f.comp_stride];
  }
  if (c == GO2NN_TRACE_REWARD) return eval_f(in.rew_buf, e, 0);
  return eval_b(c == GO2NN_TRACE_RESET ? in.reset_buf : in.time_out_buf, e) != 0 ? 1.f : 0.f;
}

#ifndef GO2_EMU
__global__ void __launch_bounds__(TRACE_THREADS) go2nn_trace_record_kernel(const Go2nnTraceIn in, const int32_t* env_ids, int K, float* frames, const int32_t* cursor, int T) {
  const int i = blockIdx.x * TRACE_THREADS + threadIdx.x;
  if (i >= K * GO2NN_TRACE_WIDTH) return;
  const int slot = (int)((uint32_t)*cursor % (uint32_t)T);
  frames[(long long)slot * K * GO2NN_TRACE_WIDTH + i] = trace_value(in, env_ids[i / GO2NN_TRACE_WIDTH], i % GO2NN_TRACE_WIDTH);
}
// <<<1, 1>>>: value < 0 sets the cursor to 0, otherwise adds `value`
__global__ void go2nn_trace_cursor_kernel(int32_t* cursor, int value) { *cursor = value < 0 ? 0 : *cursor + value; }
#endif

static int trace_in_ok(const Go2nnTraceIn* in) {
  const Go2nnEvalField* vec[] = {&in->root_states, &in->dof_state, &in->torques, &in->actions, &in->commands, &in->base_lin_vel, &in->base_ang_vel, &in->projected_gravity,
                                 &in->rigid_body_states, &in->contact_forces};
  const Go2nnEvalField* scalar[] = {&in->rew_buf, &in->reset_buf, &in->time_out_buf};
  for (const Go2nnEvalField* x : vec)
    if (!x->p || x->env_stride < 1 || x->comp_stride < 1) return 0;
  for (const Go2nnEvalField* x : scalar)
    if (!x->p || x->env_stride < 1 || x->comp_stride < 0) return 0;
  for (int f = 0; f < 4; ++f)
    if (in->foot_body[f] < 0) return 0;
  return in->dof_vel_offset >= 1 && in->rigid_body_stride >= 1 && in->contact_body_stride >= 1;
}

extern "C" {

int go2nn_trace_clear(int32_t* cursor, void* stream) {
  if (!cursor) FAIL(GO2NN_EINVAL, "trace clear: null cursor");
#ifdef GO2_EMU
  (void)stream;
  *cursor = 0;
#else
  hipLaunchKernelGGL(go2nn_trace_cursor_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, cursor, -1);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

int go2nn_trace_record(const Go2nnTraceIn* in, const int32_t* env_ids, int32_t K, float* frames, int32_t* cursor, int32_t T, void* stream) {
  if (!in || !env_ids || !frames || !cursor) FAIL(GO2NN_EINVAL, "trace record: null argument");
  if (K < 1 || T < 1 || (long long)K * GO2NN_TRACE_WIDTH > 0x7fffffffLL) FAIL(GO2NN_EINVAL, "trace record: K = %d tracked robots, T = %d slots (both >= 1)", K, T);
  if (!trace_in_ok(in))
    FAIL(GO2NN_EINVAL, "trace record: bad source (every field needs a pointer and an env stride >= 1; vector fields, the body strides and dof_vel_offset a stride >= 1)");
  const int n = K * GO2NN_TRACE_WIDTH;
#ifdef GO2_EMU
  (void)stream;
  float* slot = frames + (long long)((uint32_t)*cursor % (uint32_t)T) * n;
  for (int i = 0; i < n; ++i) slot[i] = trace_value(*in, env_ids[i / GO2NN_TRACE_WIDTH], i % GO2NN_TRACE_WIDTH);
  *cursor += 1;
#else
  hipLaunchKernelGGL(go2nn_trace_record_kernel, dim3((unsigned)((n + TRACE_THREADS - 1) / TRACE_THREADS)), dim3(TRACE_THREADS), 0, (hipStream_t)stream, *in, env_ids, K, frames,
                     cursor, T);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(go2nn_trace_cursor_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, cursor, 1);
  HIPCHK(hipGetLastError());
#endif
  return 0;
}

}  // extern "C"

#endif  // GO2NN_TRACE_H
