// DEBUGGING AID, NOT PRODUCT: the launch shape the library chooses for a search (hm355_plan_launch of hm-16.2_amd/csrc/hm355_host_common.h, which
// run_begin and lane_init of hm355.hip call), for arguments given as integers.  Nothing of the kernel source runs here.
//   hostsim_plan <wCtu> <hCtu> <wpp> <max_batch> <n> <ctu0> <ctu1> <any_inter> <fast> <env_team> <env_team_waves> <lane_share> <team_cap>
//     env_team: HM355_TEAM (-1 unset, 0, 1); env_team_waves: HM355_TEAM_WAVES (0 unset); team_cap: teams the lane has windows for
//     prints one line "name=value ..." (the fields of hm355_launch_plan)
//   hostsim_plan -
//     the same for many launches: reads records of 13 int32 (the arguments above) from stdin, writes records of 11 int32 to stdout:
//     wsCount parallel total fewWaves teamWanted waves want useTeam teams grid groups
#include "hostsim_common.h"

enum { N_IN = 13, N_OUT = 11 };

static void plan(const int32_t *a, int32_t *o)
{
  const hm355_launch_plan p = hm355_plan_launch(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12]);
  o[0] = (int32_t)p.wsCount; o[1] = (int32_t)p.parallel; o[2] = p.total; o[3] = p.fewWaves; o[4] = p.teamWanted; o[5] = p.waves; o[6] = p.want;
  o[7] = p.useTeam; o[8] = p.teams; o[9] = p.grid; o[10] = p.groups;
}

int main(int argc, char **argv)
{
  int32_t a[N_IN], o[N_OUT];
  if (argc == 2 && argv[1][0] == '-') {
    while (fread(a, sizeof(int32_t), N_IN, stdin) == N_IN) { plan(a, o); if (fwrite(o, sizeof(int32_t), N_OUT, stdout) != N_OUT) return 1; }
    return 0;
  }
  if (argc != 1 + N_IN) { fprintf(stderr, "usage: %s wCtu hCtu wpp max_batch n ctu0 ctu1 any_inter fast env_team env_team_waves lane_share team_cap | -\n", argv[0]); return 2; }
  for (int i = 0; i < N_IN; i++) a[i] = atoi(argv[1 + i]);
  plan(a, o);
  static const char *names[N_OUT] = {"wsCount", "parallel", "total", "fewWaves", "teamWanted", "waves", "want", "useTeam", "teams", "grid", "groups"};
  for (int i = 0; i < N_OUT; i++) printf("%s=%d%c", names[i], o[i], i + 1 < N_OUT ? ' ' : '\n');
  return 0;
}
