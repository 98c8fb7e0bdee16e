// Stand-ins for the kernel launchers (the sanitizer build exercises the HOST half of the C ABI only: validation, run tables,
// eligibility tests of the row kernel - pdh_check_problem / pdh_check_rows / pdh_check_exchange; nothing is launched).
#include <hip/hip_runtime.h>
struct PdhDev;
struct PdhRows;
#define S(g) extern "C" hipError_t pdh_launch_g##g(int,int,int,int,int,const PdhDev*,int,size_t,hipStream_t){return hipSuccess;}
S(0) S(1) S(2) S(3) S(4) S(5) S(6) S(7)
extern "C" hipError_t pdh_launch_rhs(int,int,const PdhDev*,int,const double*,const double*,double*,const int64_t*,const int64_t*,const int64_t*,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_eval(int,int,int,const PdhDev*,int,const double*,const int64_t*,const double*,int64_t,double*,double*,int,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_shape(int,int,const PdhDev*,int,const int64_t*,const double*,int64_t,double*,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_moment(int,int,const PdhDev*,const double*,int,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_rows(const PdhDev*,const PdhRows*,const double*,int,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_pack_faces(int,int64_t,const double*,const double*,const double*,const double*,int64_t,const int64_t*,const int64_t*,const int32_t*,const int32_t*,const double*,int64_t,double*,double*,double*,double*,double*,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_ghost_apply(const PdhDev*,const double*,int,const int64_t*,const int64_t*,const int32_t*,int,const int64_t*,const int64_t*,const int32_t*,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_checksum(const double*,int64_t,double*,hipStream_t){return hipSuccess;}
extern "C" int pdh_rows_max_faces(void){return 6;}
extern "C" int pdh_rows_n_dofs(int n1d,int basis){return basis ? n1d*(n1d+1)*(n1d+2)/6 : n1d*n1d*n1d;}
extern "C" int pdh_moment_table_doubles(int n1d){const int NA=2*n1d-1;return 3*n1d*n1d*(NA+1)+2*n1d+NA*2*n1d+2*n1d*2*n1d;}
struct PdhTerms;
extern "C" hipError_t pdh_launch_terms(const PdhDev*,const PdhTerms*,int,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_terms_gather(const PdhDev*,const PdhTerms*,double*,int,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_tiled(int,int,int,const PdhDev*,int,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_eval_err(int,int,const PdhDev*,int,const double*,const int64_t*,const double*,int64_t,const double*,const double*,const double*,double*,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_gen_volume(int,const double*,const double*,const double*,const int32_t*,int64_t,double*,int64_t,double*,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_gen_faces(int,const double*,const double*,const double*,const int32_t*,const int32_t*,int64_t,double*,double*,double*,hipStream_t){return hipSuccess;}
extern "C" int pdh_tiled_has_kind(int dim,int n1d,int){return dim == 3 && n1d >= 5 && n1d <= 8;}
// (as pdh_terms.hip: FE_DGQ(3) has the workgroup kernel, the other elements of degree 1 .. 3 the wave kernel)
extern "C" int pdh_terms_has_kind(int n1d,int basis){return (n1d < 2 || n1d > 4 || basis < 0 || basis > 1) ? 0 : (n1d == 4 && basis == 0) ? 2 : 1;}
// (any size that fits the LDS budget: the host tables of the term kernels are built in full)
extern "C" int pdh_terms_lds_bytes(int,int,int,int,int,int,int,int){return 1024;}
struct PdhSolveArgs;
extern "C" hipError_t pdh_launch_vmult(const PdhSolveArgs*,const double*,double*,double*,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_block_inverse(const PdhSolveArgs*,double*,int32_t*,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_diag_inverse(const PdhSolveArgs*,double*,int32_t*,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_cg_update(const PdhSolveArgs*,int,int,const double*,const double*,const double*,const double*,double*,double*,double*,const double*,double*,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_cg_direction(int64_t,int,const double*,double*,const double*,hipStream_t){return hipSuccess;}
extern "C" hipError_t pdh_launch_cg_finalise(const double*,int,int,double*,hipStream_t){return hipSuccess;}
extern "C" int pdh_terms_task_doubles(int maxsf,int maxcell,int pm){return (2*maxsf+3*maxcell)*3*pm+2*maxsf;}
