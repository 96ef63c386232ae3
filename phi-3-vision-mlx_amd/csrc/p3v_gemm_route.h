// The bf16 prefill GEMM family's internal interface: gemm_route (p3v_gemm.hip) decides, these launch what it decided.  None of them
// checks a shape or refuses one: `l` is a launch of a route whose status is P3V_OK, S the route's slice count (S > 1: fp32 partials
// [S, M, W rows] into a->ws, which the route found large enough).
#pragma once
#include "p3v_gemm_qkv.h"

#define P3V_EPI_QKV 100                // internal: the qkv projection with split + RoPE + KV append in the epilogue (p3v_gemm_qkv.h)

int p3v_gemm_rows_launch(const p3v_gemm_args_t* a, const p3v_gemm_launch_t& l, int S, hipStream_t s);      // p3v_gemm_rows.hip
int p3v_gemm_skinny_launch(const p3v_gemm_args_t* a, const p3v_gemm_launch_t& l, int S, hipStream_t s);    // p3v_gemm_skinny.hip
int p3v_gemm_skinny_qkv(const p3v_gemm_args_t* a, const QkvP& q, const p3v_gemm_launch_t& l, hipStream_t s);
int p3v_gemm256_launch(const p3v_gemm_args_t* a, const p3v_gemm_launch_t& l, hipStream_t s);               // p3v_gemm256.hip: a = the launch's rows
int p3v_gemm256_qkv(const p3v_gemm_args_t* a, const QkvP& q, const p3v_gemm_launch_t& l, hipStream_t s);
