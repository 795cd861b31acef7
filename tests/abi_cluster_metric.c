/* sizeof / offsetof of sg_cluster_metric for tests/test_abi_cluster_metrics.py */
#include <stddef.h>
#include <stdio.h>

#include "../include/sentinel_gpu.h"

int main(void) {
    printf("sg_cluster_metric %zu\n", sizeof(sg_cluster_metric));
    printf("cm.res_id %zu\n", offsetof(sg_cluster_metric, res_id));
    printf("cm.pass_qps %zu\n", offsetof(sg_cluster_metric, pass_qps));
    printf("cm.n_top %zu\n", offsetof(sg_cluster_metric, n_top));
    printf("cm.top_key %zu\n", offsetof(sg_cluster_metric, top_key));
    printf("cm.top_qps %zu\n", offsetof(sg_cluster_metric, top_qps));
    printf("SG_CLUSTER_TOP_MAX %d\n", SG_CLUSTER_TOP_MAX);
    printf("SG_CM_PARAM %d\n", (int)SG_CM_PARAM);
    return 0;
}
