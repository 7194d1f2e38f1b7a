#include "primme.h" /* the reference splits its interface over primme_eigs.h and primme_svds.h; here both come with primme.h */
